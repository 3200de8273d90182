"""Moving run-length masks to another pixel grid, the host definition (mrcnn_rle_transform_host; detection.rle_transform_host and the
named wrappers): the definition against the rule restated in numpy on dense planes (tests/transform_cases.py), every wrapper against
its numpy counterpart, crop after place, the capacity protocol, every argument error with its message and untouched outputs, and the
closed-form inverse of csrc/transform_rule.h (mrcnn_test_xf_preimage) against brute force.  No test here needs a GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import transform_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SHAPE, INVALID = TC.SHAPE, TC.INVALID


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


@pytest.fixture(scope="module")
def cases():
    return TC.all_cases()


def test_symbols_declared_bound_and_exported():
    lib = _mod("_lib")
    L = lib.lib()
    header = open(os.path.join(INC, "maskrcnn_hip.h")).read()
    for name in ("mrcnn_rle_transform", "mrcnn_rle_transform_host"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes and f"MRCNN_API int {name}(" in header
    assert "#define MRCNN_XF_TRANSPOSE 1\n" in header and lib.XF_TRANSPOSE == 1 == TC.TRANSPOSE
    assert "#define MRCNN_XF_MAX_BOX_WORDS (1LL << 30)\n" in header and lib.XF_MAX_BOX_WORDS == 1 << 30
    test_header = open(os.path.join(INC, "maskrcnn_hip_test.h")).read()
    assert "mrcnn_test_xf_preimage" in lib.TEST_SYMBOLS and "MRCNN_API int mrcnn_test_xf_preimage(" in test_header
    D = _mod("detection")
    for name in ("rle_transform", "rle_crop", "rle_place", "rle_flip", "rle_transpose", "rle_rot90", "rle_resize"):
        assert callable(getattr(D, name)) and callable(getattr(D, name + "_host"))


# ---- 1. the definition against the numpy rule ------------------------------------------------------------------------------------------------
def test_every_case_equals_the_numpy_rule(cases):
    """one ragged call over all cases; out_counts, out_run_offsets, areas and bboxes_xywh against the planes of the restatement"""
    names = cases["names"]
    assert 200 < len(names) < 3000 and len({(h, w) for h, w in zip(cases["hs"], cases["ws"])}) == len(TC.SIZES)
    assert any((c[1:] == 0).any() for c in cases["runs"])                           # zero-length runs are in
    flags = cases["xf"][:, 0]
    assert (flags == 1).sum() > 100 and (flags == 0).sum() > 100                    # transposed and plain records
    assert (cases["xf"][:, [1, 4]] < 0).any() and (cases["xf"][:, [2, 5]] < 0).any()
    st, msg, out, offs, areas, boxes = TC.transform_host(*TC.flat_set(cases["runs"]), cases["hs"], cases["ws"], cases["ohs"], cases["ows"], cases["xf"])
    assert st == 0, msg
    empties = fulls = 0
    for k, name in enumerate(names):
        want = TC.reference(cases["planes"][k], cases["xf"][k], int(cases["ohs"][k]), int(cases["ows"][k]))
        got = out[int(offs[k]):int(offs[k + 1])]
        assert got.tolist() == TC.encode(want).tolist(), name
        assert (int(areas[k]), boxes[k].tolist()) == TC.stats(want), name
        assert (got[1:] > 0).all(), name                                            # canonical: only counts[0] may be 0
        empties += want.sum() == 0
        fulls += bool(want.all())
        if name.startswith("crop_outside/"):
            assert got.tolist() == [want.size], name
    assert empties > 0 and fulls > 0


def test_the_restatement_is_the_rule_pixel_by_pixel():
    """the numpy gather itself against the rule as the header reads, with Python's integers, on a plane small enough to loop over"""
    rng = np.random.default_rng(5)
    P = (rng.random((6, 9)) < 0.5).astype(np.uint8)
    for name, r, (oh, ow) in TC.records_of(6, 9, rng):
        want = np.zeros((oh, ow), np.uint8)
        flags, ax, bx, dx, ay, by, dy, _ = (int(v) for v in r)
        for Y in range(oh):
            for X in range(ow):
                u, v = (ax * X + bx) // dx, (ay * Y + by) // dy
                sx, sy = (v, u) if flags & 1 else (u, v)
                if 0 <= sx < 9 and 0 <= sy < 6:
                    want[Y, X] = P[sy, sx]
        assert (TC.reference(P, r, oh, ow) == want).all(), name


# ---- 2. the wrappers -----------------------------------------------------------------------------------------------------------------------
def _rows():
    """two images of different sizes, three masks each: an ellipse, a random plane re-encoded with zero-length runs, the comb"""
    from morph_cases import ellipse
    rng = np.random.default_rng(47)
    sizes = [(40, 70), (65, 33)]
    planes, rows = [], []
    for h, w in sizes:
        comb = np.zeros((h, w), np.uint8); comb[:, ::2] = 1; comb[0, :] = 1
        ps = [ellipse(h, w, h * 0.4, w * 0.6, h * 0.3, w * 0.25), (rng.random((h, w)) < 0.5).astype(np.uint8), comb]
        planes.append(ps)
        rows.append([{"size": [h, w], "counts": TC.with_zero_runs(TC.encode(p), rng) if i == 1 else TC.encode(p)} for i, p in enumerate(ps)])
    return rows, planes, sizes


def _same(got, want_planes, what):
    rle, areas, boxes, _sizes = got
    for b, row in enumerate(want_planes):
        for i, want in enumerate(row):
            assert rle[b][i]["size"] == list(want.shape), (what, b, i)
            assert rle[b][i]["counts"].tolist() == TC.encode(want).tolist(), (what, b, i)
            assert (int(areas[b, i]), boxes[b, i].tolist()) == TC.stats(want), (what, b, i)


def test_the_named_wrappers_against_numpy():
    D = _mod("detection")
    rows, planes, sizes = _rows()
    # crop: slicing a zero-padded plane; one window for all, and one per image that reaches outside on every side
    pad = 20
    for windows in ([(5, 7, 20, 11)], [(-3, -4, 80, 50), (30, 60, 9, 9)]):
        per = windows * 2 if len(windows) == 1 else windows
        want = [[np.pad(p, pad)[y + pad:y + pad + wh, x + pad:x + pad + ww] for p in row] for row, (x, y, ww, wh) in zip(planes, per)]
        got = D.rle_crop_host(rows, None, windows)
        _same(got, want, "crop")
        assert got[3] == [(wh, ww) for (_, _, ww, wh) in per]
    # place: np.pad
    got = D.rle_place_host(rows, None, [(4, 9)], [(90, 100)])
    _same(got, [[np.pad(p, ((9, 90 - 9 - p.shape[0]), (4, 100 - 4 - p.shape[1]))) for p in row] for row in planes], "place")
    assert got[3] == [(90, 100), (90, 100)]
    # flips: np.flip
    for hz, vt in ((True, False), (False, True), (True, True), (False, False)):
        axes = tuple(a for a, on in ((1, hz), (0, vt)) if on)
        _same(D.rle_flip_host(rows, None, horizontal=hz, vertical=vt), [[np.flip(p, axes) if axes else p for p in row] for row in planes], f"flip {hz} {vt}")
    # rotations: np.rot90, and past a full turn
    for k in (0, 1, 2, 3, 5, -1):
        got = D.rle_rot90_host(rows, None, k)
        _same(got, [[np.rot90(p, k) for p in row] for row in planes], f"rot90 {k}")
        assert got[3] == [np.rot90(row[0], k).shape for row in planes]
    _same(D.rle_transpose_host(rows), [[p.T for p in row] for row in planes], "transpose")
    # resize: the two published index rules
    for rule, index in (("center", lambda X, n, N: ((2 * X + 1) * n) // (2 * N)), ("floor", lambda X, n, N: (X * n) // N)):
        for oh, ow in ((20, 35), (97, 41), (1, 1)):
            want = [[p[np.ix_(index(np.arange(oh), p.shape[0], oh), index(np.arange(ow), p.shape[1], ow))] for p in row] for row in planes]
            _same(D.rle_resize_host(rows, None, [(oh, ow)], rule), want, f"resize {rule} {oh}x{ow}")
    with pytest.raises(ValueError):
        D.rle_resize_host(rows, None, [(20, 35)], "bilinear")
    with pytest.raises(ValueError):
        D.rle_resize_host(rows, None, [(0, 35)])
    with pytest.raises(ValueError):
        D.rle_crop_host(rows, None, [(0, 0, 5, 5)] * 4)                             # neither one, one per size nor one per RLE


def test_a_pair_in_is_a_pair_out_and_sizes_come_back():
    D = _mod("detection")
    rows, planes, sizes = _rows()
    pair = TC.flat_set([e["counts"] for r in rows for e in r])
    (c, o), areas, boxes, new = D.rle_rot90_host(pair, sizes, 1)
    assert new == [(70, 40), (33, 65)] and len(o) == 7 and areas.shape == (6,) and boxes.shape == (6, 4)
    want = [TC.encode(np.rot90(p)) for row in planes for p in row]
    assert c.tolist() == np.concatenate(want).tolist()
    # one record per RLE and planes that differ inside an image: the sizes come back per RLE
    windows = [(0, 0, 3 + k, 2 + k) for k in range(6)]
    (c, o), _, _, new = D.rle_crop_host(pair, sizes, windows)
    assert new == [(2 + k, 3 + k) for k in range(6)]
    want = [TC.encode(p[:2 + k, :3 + k]) for k, p in enumerate(p for row in planes for p in row)]
    assert c.tolist() == np.concatenate(want).tolist()
    # rle_transform itself: one record for all
    (c, o), _, _, new = D.rle_transform_host(pair, sizes, [0, 1, 2, 1, 1, 3, 1, 0], [(10, 12)])
    want = [TC.encode(p[3:13, 2:14]) for row in planes for p in row]
    assert c.tolist() == np.concatenate(want).tolist() and new == [(10, 12)] * 2
    (c, o), areas, _, new = D.rle_flip_host((np.zeros(0, np.uint32), np.zeros(1, np.int64)), [], horizontal=True)      # no RLE
    assert len(c) == 0 and o.tolist() == [0] and len(areas) == 0 and new == []


def test_crop_after_place_is_the_identity_and_zero_runs_become_canonical():
    D = _mod("detection")
    rows, planes, sizes = _rows()
    placed, _, _, frame = D.rle_place_host(rows, None, [(13, 8), (0, 31)], [(120, 110)])
    assert frame == [(120, 110)] * 2
    back, areas, _, new = D.rle_crop_host(placed, None, [(13, 8, 70, 40), (0, 31, 33, 65)])
    assert new == sizes
    assert (rows[0][1]["counts"][1:] == 0).any()                                     # an input with zero-length runs
    for b, row in enumerate(planes):
        for i, p in enumerate(row):
            assert back[b][i]["counts"].tolist() == TC.encode(p).tolist() and int(areas[b, i]) == int(p.sum())
    same, _, _, _ = D.rle_flip_host(rows)                                            # the identity record: the canonical RLE of the same plane
    assert [[e["counts"].tolist() for e in r] for r in same] == [[TC.encode(p).tolist() for p in row] for row in planes]


# ---- 3. capacity, errors -------------------------------------------------------------------------------------------------------------------
def _three():
    from morph_cases import ellipse
    planes = [ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), ellipse(20, 30, 12, 12, 5, 5), ellipse(7, 5, 3, 2, 2, 1)]
    runs = [TC.encode(p) for p in planes]
    xf = np.stack([TC.symmetry(20, 30, 1, 0, 1)[0], TC.crop(-1, -1, 8, 9)[0], TC.resize(20, 30, 30, 45, "center")[0], TC.crop(9, 0, 2, 2)[0]])
    ohs, ows = np.array([30, 9, 30, 2], np.int32), np.array([20, 8, 45, 2], np.int32)
    return planes, *TC.flat_set(runs), np.array([20, 7, 20, 7], np.int32), np.array([30, 5, 30, 5], np.int32), ohs, ows, xf


def test_size_query_small_capacity_and_no_rle():
    planes, counts, offs, hs, ws, ohs, ows, xf = _three()
    st, msg, want, want_offs, want_areas, want_boxes = TC.transform_host(counts, offs, hs, ws, ohs, ows, xf)
    assert st == 0, msg
    need = int(want_offs[4])
    assert want_areas.tolist() == [int(planes[0].sum()), 35, int(TC.reference(planes[2], xf[2], 30, 45).sum()), 0]
    assert want[int(want_offs[3]):].tolist() == [4]                                  # the window wholly outside: the empty RLE [H'*W']
    L = _mod("_lib").lib()
    p = lambda a: a.ctypes.data
    o, a, b = np.full(5, 77, np.int64), np.full(4, 77, np.uint32), np.full((4, 4), 77, np.int32)
    head = (p(counts), p(offs), 4, p(hs), p(ws), p(ohs), p(ows), p(xf))
    assert L.mrcnn_rle_transform_host(*head, None, 0, p(o), p(a), p(b)) == SHAPE     # the size query: capacity 0, out_counts NULL
    msg = L.mrcnn_last_error().decode()
    assert msg.startswith("rle_transform_host:") and f"capacity >= {need}" in msg
    assert o.tolist() == want_offs.tolist() and a.tolist() == want_areas.tolist() and (b == want_boxes).all()
    out = np.full(need + 5, 77, np.uint32)
    assert L.mrcnn_rle_transform_host(*head, p(out), need - 1, p(o), None, None) == SHAPE and (out == 77).all()
    assert f"holds {need - 1}: call again with capacity >= {need}" in L.mrcnn_last_error().decode()
    assert L.mrcnn_rle_transform_host(*head, p(out), need + 5, p(o), None, None) == 0
    assert out[:need].tolist() == want.tolist() and (out[need:] == 77).all()
    one, zero = np.full(1, 77, np.int64), np.zeros(1, np.int64)
    assert L.mrcnn_rle_transform_host(None, p(zero), 0, None, None, None, None, None, None, 0, p(one), None, None) == 0          # n = 0
    assert one.tolist() == [0]


def _raw(entry_host, counts, offs, n, hs, ws, ohs, ows, xf, capacity=64, memspace=0, nulls=()):
    """either entry (the device entry with host pointers: argument errors need no device) with pre-filled outputs ->
    (status, message, [out_counts, out_run_offsets, areas, bboxes])"""
    L = _mod("_lib").lib()
    bufs = [np.full(max(1, capacity), 77, np.uint32), np.full(max(1, n) + 1, 77, np.int64), np.full(max(1, n), 77, np.uint32), np.full((max(1, n), 4), 77, np.int32)]
    p = lambda name, a: None if name in nulls or a is None else np.ascontiguousarray(a).ctypes.data
    keep = [np.ascontiguousarray(a) for a in (counts, offs, hs, ws, ohs, ows, xf)]
    head = (p("counts", keep[0]), p("run_offsets", keep[1]), n, p("heights", keep[2]), p("widths", keep[3]), p("out_heights", keep[4]), p("out_widths", keep[5]),
            p("xf", keep[6]))
    tail = (p("out_counts", bufs[0]), capacity, p("out_run_offsets", bufs[1]), p("areas", bufs[2]), p("bboxes", bufs[3]))
    st = L.mrcnn_rle_transform_host(*head, *tail) if entry_host else L.mrcnn_rle_transform(*head, memspace, *tail)
    return st, L.mrcnn_last_error().decode(), bufs


@pytest.mark.parametrize("entry_host", [True, False], ids=["rle_transform_host", "rle_transform"])
def test_errors_and_untouched_outputs(entry_host):
    who = "rle_transform_host:" if entry_host else "rle_transform:"
    _planes, counts, offs, hs, ws, ohs, ows, xf = _three()

    def refused(code, text, **kw):
        args = dict(counts=counts, offs=offs, n=4, hs=hs, ws=ws, ohs=ohs, ows=ows, xf=xf)
        args.update(kw)
        st, msg, bufs = _raw(entry_host, *(args[k] for k in ("counts", "offs", "n", "hs", "ws", "ohs", "ows", "xf")),
                             **{k: v for k, v in args.items() if k in ("capacity", "memspace", "nulls")})
        assert st == code and msg.startswith(who) and text in msg, (st, msg)
        assert all((b == 77).all() for b in bufs), msg

    for name in ("run_offsets", "heights", "widths", "out_heights", "out_widths", "xf", "out_run_offsets", "out_counts"):
        refused(INVALID, "null", nulls=(name,))
    if not entry_host:
        refused(INVALID, "unknown memspace 7", memspace=7)
    refused(SHAPE, "n -1 is negative", n=-1)
    for bad_side in (0, 32768):
        h2 = hs.copy(); h2[3] = bad_side
        refused(SHAPE, f"RLE 3 is {bad_side}x5: height and width must lie in 1..32767", hs=h2)
        w2 = ws.copy(); w2[1] = bad_side
        refused(SHAPE, f"RLE 1 is 7x{bad_side}", ws=w2)
        oh2 = ohs.copy(); oh2[2] = bad_side
        refused(SHAPE, f"RLE 2 goes to a {bad_side}x45 plane: height and width must lie in 1..32767", ohs=oh2)
        ow2 = ows.copy(); ow2[0] = bad_side
        refused(SHAPE, f"RLE 0 goes to a 30x{bad_side} plane", ows=ow2)
    down = offs.copy(); down[2] = down[1] - 1
    refused(SHAPE, "run_offsets decrease at RLE 1", offs=down)

    def record(k, word, value):
        x = xf.copy(); x[k, word] = value
        return x

    refused(SHAPE, "RLE 1 has flags 2", xf=record(1, 0, 2))
    refused(SHAPE, "RLE 0 has flags 3", xf=record(0, 0, 3))
    refused(SHAPE, "RLE 2 has flags -1", xf=record(2, 0, -1))
    refused(SHAPE, "RLE 3 has 5 in word 7", xf=record(3, 7, 5))
    for word, axis in ((1, "ax, bx, dx"), (4, "ay, by, dy")):
        refused(SHAPE, f"RLE 1 has {axis} = 0,", xf=record(1, word, 0))                              # a = 0
        refused(SHAPE, f"RLE 1 has {axis} = {2 ** 31},", xf=record(1, word, 2 ** 31))
        refused(SHAPE, f"RLE 1 has {axis} = {-2 ** 31},", xf=record(1, word, -2 ** 31))
        refused(SHAPE, f"RLE 2 has {axis} =", xf=record(2, word + 1, 2 ** 46 + 1))                   # b
        refused(SHAPE, f"RLE 2 has {axis} =", xf=record(2, word + 1, -2 ** 46 - 1))
        refused(SHAPE, f"RLE 3 has {axis} = 1, {9 if word == 1 else 0}, 0:", xf=record(3, word + 2, 0))      # d
        refused(SHAPE, f"RLE 3 has {axis} =", xf=record(3, word + 2, -1))
        refused(SHAPE, f"RLE 3 has {axis} =", xf=record(3, word + 2, 2 ** 31))
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1 and RLE 3: the lowest is named
    bad[int(offs[3])] -= 1
    if entry_host:                                               # (the device entry finds a wrong total on the device: tests/test_gpu_rle_transform.py)
        refused(SHAPE, "RLE 1 sums to 38 pixels, its 7x5 plane has 35", counts=bad)


def test_the_limits_themselves_are_legal():
    """a record at the coefficient limits is accepted and follows the rule: no product leaves int64"""
    P = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
    big, b = 2 ** 31 - 1, 2 ** 46
    xf = np.array([[0, big, -10 * big, big, -big, 12 * big, big, 0],         # u = X - 10, v = 12 - Y
                   [1, -big, b, 1, big, -b, 1, 0]], np.int64)                # every source index far outside: the empty mask
    counts, offs = TC.flat_set([TC.encode(P)] * 2)
    ohs, ows = np.array([40, 50], np.int32), np.array([50, 40], np.int32)
    st, msg, out, o, areas, _ = TC.transform_host(counts, offs, [3, 3], [2, 2], ohs, ows, xf)
    assert st == 0, msg
    for k in range(2):
        want = TC.reference(P, xf[k], int(ohs[k]), int(ows[k]))
        assert out[int(o[k]):int(o[k + 1])].tolist() == TC.encode(want).tolist() and int(areas[k]) == int(want.sum())


# ---- 4. the inverse ------------------------------------------------------------------------------------------------------------------------
def test_the_closed_form_preimage_equals_brute_force():
    """csrc/transform_rule.h's xf_preimage: the X with a <= floor((A*X + B)/D) < b are exactly [lo, hi), over a range of X wide enough to hold them"""
    L = _mod("_lib").lib()
    lo, hi = C.c_int64(0), C.c_int64(0)
    X = np.arange(-200, 201)
    checked = empty = 0
    for A in (1, 2, 3, 5, 7, -1, -2, -3, -5, -7):
        for D in (1, 2, 3, 7):
            for B in range(-20, 21):
                u = (A * X + B) // D                                 # numpy's // on integers: floor
                for a in range(-3, 7):
                    for b in range(a, 7):
                        assert L.mrcnn_test_xf_preimage(a, b, A, B, D, C.byref(lo), C.byref(hi)) == 0
                        inside = X[(u >= a) & (u < b)]
                        if inside.size:
                            assert (lo.value, hi.value) == (int(inside[0]), int(inside[-1]) + 1) and inside.size == hi.value - lo.value, (a, b, A, B, D)
                        else:
                            assert lo.value >= hi.value, (a, b, A, B, D)
                            empty += 1
                        checked += 1
    assert checked > 50000 and empty > 1000
    assert L.mrcnn_test_xf_preimage(0, 1, 0, 0, 1, C.byref(lo), C.byref(hi)) == SHAPE
    assert L.mrcnn_test_xf_preimage(2, 1, 1, 0, 1, C.byref(lo), C.byref(hi)) == SHAPE
    assert L.mrcnn_test_xf_preimage(0, 1, 1, 0, 1, None, C.byref(hi)) == INVALID
