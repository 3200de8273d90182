"""Connected components of run-length masks, the host definition (mrcnn_rle_components_host, mrcnn_rle_components_select_host and
detection's _host helpers): no GPU.  Every case of tests/components_cases.py against the pixel union-find restated there, for both
values and both connectivities; identities of the 4 / 8 duality checked on the polygon tracer's host definition, which was written
without any of this; the identities of MERGE and SPLIT; errors and the two capacity protocols."""
import ctypes as C
import importlib

import numpy as np
import pytest

import components_cases as CC
import morph_cases as MC

SHAPE, INVALID, HIP = CC.SHAPE, CC.INVALID, CC.HIP


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


@pytest.fixture(scope="module")
def cases(pkg):
    return CC.all_cases()


@pytest.fixture(scope="module")
def labelled(cases):
    """the host entry's measures of all cases in one ragged call, per (of, connectivity)"""
    out = {}
    for of, conn in CC.COMBOS:
        st, msg, *arrays = CC.components_host(*CC.flat_set(cases), conn, of)
        assert st == 0, msg
        out[of, conn] = arrays
    return out


def test_symbols_exported(pkg):
    lib = _mod("_lib")
    for s in ("mrcnn_rle_components", "mrcnn_rle_components_host", "mrcnn_rle_components_select", "mrcnn_rle_components_select_host"):
        assert s in lib.EXPORTED_SYMBOLS and hasattr(lib.lib(), s)


def test_the_cases_are_what_they_claim(cases, labelled):
    assert len(cases) > 500
    by = {c[0]: c for c in cases}
    at = {c[0]: k for k, c in enumerate(cases)}
    found = lambda name, of, conn: int(np.diff(labelled[of, conn][0])[at[name]])              # what the host entry counts in that case
    assert [found("spiral_33", 1, 4), found("two_spirals_41", 1, 8), found("diagonal_pair", 1, 4), found("diagonal_pair", 1, 8)] == [1, 2, 2, 1]
    assert [found("diagonal_line", 0, 4), found("diagonal_line", 0, 8), found("rings_21", 1, 4), found("rings_21", 0, 4)] == [1, 2, 4, 4]
    assert [found("bottom_beside_top", 1, 8), found("row_run_over_five_columns", 1, 4)] == [2, 1]
    assert [found(f"pieces_{c}", 1, 4) for c in (CC.PIECES_THRESHOLD - 1, CC.PIECES_THRESHOLD, CC.PIECES_THRESHOLD + 1)] == \
        [CC.PIECES_THRESHOLD - 1, CC.PIECES_THRESHOLD, CC.PIECES_THRESHOLD + 1]
    assert CC.label(by["spiral_33"][4], 4, CC.ONES)[1] == 1 and CC.label(by["spiral_33"][4], 4, CC.ZEROS)[1] == 1
    assert CC.label(by["two_spirals_41"][4], 8, CC.ONES)[1] == 2
    assert CC.label(by["diagonal_pair"][4], 4, CC.ONES)[1] == 2 and CC.label(by["diagonal_pair"][4], 8, CC.ONES)[1] == 1
    assert CC.label(by["diagonal_line"][4], 4, CC.ZEROS)[1] == 1 and CC.label(by["diagonal_line"][4], 8, CC.ZEROS)[1] == 2      # the dual
    assert CC.label(by["rings_21"][4], 4, CC.ONES)[1] == 4 and CC.label(by["rings_21"][4], 4, CC.ZEROS)[1] == 4
    assert CC.label(by["bottom_beside_top"][4], 8, CC.ONES)[1] == 2
    assert CC.label(by["row_run_over_five_columns"][4], 4, CC.ONES)[1] == 1
    for c in (CC.PIECES_THRESHOLD - 1, CC.PIECES_THRESHOLD, CC.PIECES_THRESHOLD + 1):
        assert CC.label(by[f"pieces_{c}"][4], 4, CC.ONES)[1] == c
    assert sum(1 for c in cases if c[0].endswith("/zero_runs")) > 200


@pytest.mark.parametrize("of,conn", CC.COMBOS)
def test_every_case_equals_the_restatement(cases, labelled, of, conn):
    offs, areas, boxes, flags = labelled[of, conn]
    assert offs[0] == 0
    for k, (name, _counts, _h, _w, plane) in enumerate(cases):
        a, b, f = CC.measures(plane, conn, of)
        lo, hi = int(offs[k]), int(offs[k + 1])
        what = f"{name}, of {of}, connectivity {conn}"
        assert hi - lo == len(a), f"{what}: {hi - lo} components, the restatement finds {len(a)}"
        CC.assert_same((areas[lo:hi], boxes[lo:hi], flags[lo:hi]), (a, b, f), ("comp_areas", "comp_bboxes_xywh", "comp_flags"), what)


def test_scipy_agrees_when_it_is_there(cases, labelled):
    ndimage = pytest.importorskip("scipy.ndimage")
    for k, (name, _c, _h, _w, plane) in list(enumerate(cases))[::7]:
        for conn, structure in ((4, None), (8, np.ones((3, 3)))):
            _, n = ndimage.label(plane, structure)
            assert n == CC.label(plane, conn, CC.ONES)[1] == int(np.diff(labelled[CC.ONES, conn][0])[k]), name


# ---- theorems of the 4 / 8 duality, on the tracer's host definition -----------------------------------------------------------------------
def test_components_are_the_traced_outlines_and_holes(cases, labelled):
    D = _mod("detection")
    rows = [[{"size": [h, w], "counts": c}] for _n, c, h, w, _p in cases]
    _rings, ring_areas, nesting = D.rle_to_polygons_host(rows, nest=True)
    o1, a1, _b1, _f1 = labelled[CC.ONES, 4]
    o0, _a0, _b0, f0 = labelled[CC.ZEROS, 4]
    for k, case in enumerate(cases):
        signed = np.asarray(ring_areas[k][0], np.int64)
        polys = nesting["nest"][k][0]
        assert int(o1[k + 1] - o1[k]) == len(polys) == int((nesting["depth"][k][0] % 2 == 0).sum()), case[0]
        assert sorted(int(signed[p].sum()) for p in polys) == sorted(a1[int(o1[k]):int(o1[k + 1])].tolist()), case[0]      # shell + its holes
        inner = int((f0[int(o0[k]):int(o0[k + 1])] & 1 == 0).sum())
        assert inner == int((signed < 0).sum()), case[0]


# ---- MERGE and SPLIT ---------------------------------------------------------------------------------------------------------------------
def _select(cases, labelled, of, conn, keep, mode):
    st, msg, *out = CC.select_host(*CC.flat_set(cases), conn, of, keep, mode)
    assert st == 0, msg
    return out


@pytest.mark.parametrize("of,conn", CC.COMBOS)
def test_merge_equals_the_restatement_and_its_identities(cases, labelled, of, conn):
    offs = labelled[of, conn][0]
    n_comps = int(offs[-1])
    rng = np.random.default_rng(3)
    canonical = [MC.encode(c[4]) for c in cases]
    for which, keep in (("all", np.ones(n_comps, np.uint8)), ("none", np.zeros(n_comps, np.uint8)), ("random", (rng.random(n_comps) < 0.5).astype(np.uint8))):
        counts, o, areas, boxes, parent = _select(cases, labelled, of, conn, keep, CC.MERGE)
        assert parent.tolist() == list(range(len(cases)))
        for k, (name, _c, h, w, plane) in enumerate(cases):
            got = counts[int(o[k]):int(o[k + 1])]
            if which == "all":
                want_plane = plane
                assert got.tolist() == canonical[k].tolist(), f"{name}: all kept is not the canonical input"
            elif which == "none":
                want_plane = np.full((h, w), 1 - of, np.uint8)
            else:
                want_plane = CC.merged(plane, conn, of, keep[int(offs[k]):int(offs[k + 1])])
            assert got.tolist() == MC.encode(want_plane).tolist(), f"{name}, {which}, of {of}, connectivity {conn}"
            area, box = MC.stats(want_plane)
            assert int(areas[k]) == area and boxes[k].tolist() == box, f"{name}, {which}: area / box"


@pytest.mark.parametrize("conn", [4, 8])
def test_split_equals_the_restatement_and_its_identities(cases, labelled, conn):
    offs = labelled[CC.ONES, conn][0]
    n_comps = int(offs[-1])
    rng = np.random.default_rng(4)
    for which, keep in (("all", np.ones(n_comps, np.uint8)), ("random", (rng.random(n_comps) < 0.4).astype(np.uint8))):
        counts, o, areas, boxes, parent = _select(cases, labelled, CC.ONES, conn, keep, CC.SPLIT)
        assert len(parent) == int(keep.sum()) and (np.diff(parent) >= 0).all()
        j = 0
        for k, (name, _c, h, w, plane) in enumerate(cases):
            wants = CC.split_counts(plane, conn, keep[int(offs[k]):int(offs[k + 1])])
            few = len(wants) <= 40                                   # the decoded planes of the cases with few components, the sums of all
            if few:
                planes = CC.split(plane, conn, keep[int(offs[k]):int(offs[k + 1])])
                union = np.zeros((h, w), np.int32)
            total = 0
            for i, want in enumerate(wants):
                assert int(parent[j]) == k, name
                got = counts[int(o[j]):int(o[j + 1])]
                assert got.tolist() == want.tolist(), f"{name}, output {j}, connectivity {conn}"
                assert int(areas[j]) == int(want[1::2].sum()), f"{name}, output {j}: area"
                total += int(areas[j])
                if few:
                    assert want.tolist() == MC.encode(planes[i]).tolist(), f"{name}: the two restatements differ"
                    area, box = MC.stats(planes[i])
                    assert int(areas[j]) == area and boxes[j].tolist() == box, f"{name}, output {j}: area / box"
                    union += MC.decode(got, h, w)
                j += 1
            if few:
                assert union.max(initial=0) <= 1, f"{name}: the outputs overlap"
            if which == "all":
                assert total == int(plane.sum()), f"{name}: the outputs do not add up to the input"
                if few:
                    assert (union == plane).all(), f"{name}: the outputs do not OR to the input"
        assert j == len(parent)
        if which == "all":                                       # every output has exactly one component when labelled again
            small = [j for j, p in enumerate(parent) if cases[int(p)][2] * cases[int(p)][3] <= 20000]       # (a plane per output: the small planes)
            runs = [counts[int(o[j]):int(o[j + 1])] for j in small]
            again_offs = np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64)
            st, msg, again, *_ = CC.components_host(np.concatenate(runs), again_offs, [cases[int(parent[j])][2] for j in small],
                                                    [cases[int(parent[j])][3] for j in small], conn, CC.ONES)
            assert st == 0 and len(small) > 3000 and (np.diff(again) == 1).all(), msg


# ---- detection's helpers -----------------------------------------------------------------------------------------------------------------
def _pair(cases):
    counts, offs, hs, ws = CC.flat_set(cases)
    return (counts, offs), list(zip(hs.tolist(), ws.tolist()))


def test_the_helpers_on_the_host(cases, labelled):
    D = _mod("detection")
    some = [c for c in cases if c[2] * c[3] <= 70 * 140][:160] + [c for c in cases if c[0].startswith("random_0.5")]
    pair, sizes = _pair(some)
    offs, areas, boxes, flags = D.rle_components_host(pair, sizes)
    st, msg, *want = CC.components_host(*CC.flat_set(some), 4, CC.ONES)
    CC.assert_same((offs, areas, boxes, flags), want, ("comp_offsets", "areas", "bboxes", "flags"), "rle_components_host")

    once = D.rle_remove_small_host(pair, sizes, 5)
    twice = D.rle_remove_small_host(once, sizes, 5)
    CC.assert_same(twice, once, ("counts", "run_offsets"), "rle_remove_small twice")
    largest = D.rle_keep_largest_host(pair, sizes, 2)
    filled = D.rle_fill_holes_host(pair, sizes)
    bounded = D.rle_fill_holes_host(pair, sizes, max_area=3)
    for k, (name, _c, h, w, plane) in enumerate(some):
        L, n = CC.label(plane, 4, CC.ONES)
        a = CC.measures(plane, 4, CC.ONES)[0].astype(np.int64)
        got = lambda p: p[0][int(p[1][k]):int(p[1][k + 1])].tolist()
        assert got(once) == MC.encode(CC.merged(plane, 4, CC.ONES, a >= 5)).tolist(), name
        order = sorted(range(n), key=lambda c: (-a[c], c))[:2]                                         # ties go to the earlier component
        assert got(largest) == MC.encode(CC.merged(plane, 4, CC.ONES, np.isin(np.arange(n), order))).tolist(), name
        za, _zb, zf = CC.measures(plane, 4, CC.ZEROS)
        assert got(filled) == MC.encode(CC.merged(plane, 4, CC.ZEROS, zf & 1 != 0)).tolist(), name
        assert got(bounded) == MC.encode(CC.merged(plane, 4, CC.ZEROS, (zf & 1 != 0) | (za > 3))).tolist(), name

    (sc, so), parent = D.rle_split_components_host(pair, sizes, min_area=4, connectivity=8)
    a8 = D.rle_components_host(pair, sizes, connectivity=8)
    assert len(parent) == int((a8[1] >= 4).sum()) == len(so) - 1
    rows = D.rle_rows_of(pair, sizes)                            # rows in, rows out
    r_rows, r_areas, r_boxes = D.rle_select_components_host(rows, None, np.ones(len(areas), np.uint8))
    assert len(r_rows) == len(some) and r_areas.shape == (len(some), 1) and r_boxes.shape == (len(some), 1, 4)
    assert all(r_rows[k][0]["counts"].tolist() == MC.encode(some[k][4]).tolist() for k in range(len(some)))
    s_rows, _sa, _sb, s_par = D.rle_select_components_host(rows, None, np.ones(len(areas), np.uint8), mode="split")
    assert len(s_rows) == len(areas) == len(s_par) and s_rows[0]["size"] == [some[int(s_par[0])][2], some[int(s_par[0])][3]]
    with pytest.raises(ValueError):
        D.rle_components_host(pair, sizes, of="twos")
    with pytest.raises(ValueError):
        D.rle_select_components_host(pair, sizes, np.ones(len(areas), np.uint8), mode="cut")


def test_a_split_past_the_first_guess_takes_the_wrappers_second_attempt(pkg, monkeypatch):
    """A run of ones that wraps from the bottom of a column into the top of the next is one run of the input and a run each of two
    components.  The top and the bottom row of a 3 x 8 plane: 18 runs and two components, so the wrapper guesses 18 + 2 * 2 + 2 = 24,
    and the two rows, a run per column each, hold 17 + 16 = 33."""
    D, L = _mod("detection"), _mod("_lib").lib()
    plane = np.zeros((3, 8), np.uint8)
    plane[[0, 2]] = 1
    runs = MC.encode(plane)
    assert len(runs) == 18
    entry, capacities = L.mrcnn_rle_components_select_host, []
    monkeypatch.setattr(L, "mrcnn_rle_components_select_host", lambda *a: capacities.append(a[11]) or entry(*a))
    (counts, offs), parent = D.rle_split_components_host((runs, np.array([0, 18], np.int64)), [(3, 8)])
    assert capacities == [24, 33]
    top, bottom = plane.copy(), plane.copy()
    top[2], bottom[0] = 0, 0
    assert counts.tolist() == MC.encode(top).tolist() + MC.encode(bottom).tolist() and offs.tolist() == [0, 17, 33] and parent.tolist() == [0, 0]


# ---- errors and capacities ---------------------------------------------------------------------------------------------------------------
def _three():
    planes = [MC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), CC.rings(16)]
    runs = [MC.encode(p) for p in planes]
    return planes, np.concatenate(runs), np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64), [20, 7, 16], [30, 5, 16]


def test_size_queries_and_capacities(pkg):
    planes, counts, offs, hs, ws = _three()
    L = _mod("_lib").lib()
    st, msg, comp_offs, areas, boxes, flags = CC.components_host(counts, offs, hs, ws, 4, CC.ONES, capacity=2, fill=77)
    assert st == SHAPE and msg.startswith("rle_components_host:") and "comp_capacity >= 5" in msg, msg
    assert comp_offs.tolist() == [0, 1, 2, 5] and (areas == 77).all() and (boxes == 77).all() and (flags == 77).all()
    st, msg, comp_offs, areas, boxes, flags = CC.components_host(counts, offs, hs, ws, 4, CC.ONES)
    assert st == 0 and len(areas) == 5 and areas[1] == 35 and boxes[1].tolist() == [0, 0, 5, 7] and flags.tolist() == [0, 1, 1, 0, 0]
    keep = np.array([1, 1, 0, 1, 1], np.uint8)
    want = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, keep, CC.MERGE)
    assert want[0] == 0
    small = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, keep, CC.MERGE, capacity=len(want[2]) - 1)
    assert small[0] == SHAPE and small[1].startswith("rle_components_select_host:") and f"capacity >= {len(want[2])}" in small[1]
    assert (small[2] == 0).all() and small[3].tolist() == want[3].tolist() and small[4].tolist() == want[4].tolist()
    split = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, keep, CC.SPLIT)
    assert split[0] == 0 and split[6].tolist() == [0, 1, 2, 2] and len(split[3]) == 5
    st, msg, *_ = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, keep[:4], CC.MERGE)
    assert st == SHAPE and "n_comps = 4" in msg and "5 components" in msg, msg
    # n = 0 is legal
    st, msg, comp_offs, *_ = CC.components_host(np.zeros(1, np.uint32), np.zeros(1, np.int64), [], [], 4, CC.ONES)
    assert st == 0 and comp_offs.tolist() == [0]
    st, msg, out, o, *_ = CC.select_host(np.zeros(1, np.uint32), np.zeros(1, np.int64), [], [], 4, CC.ONES, [], CC.MERGE, capacity=4)
    assert st == 0 and o.tolist() == [0], msg


def test_errors_and_untouched_outputs(pkg):
    _planes, counts, offs, hs, ws = _three()
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3
    bad[int(offs[2])] += 1
    st, msg, comp_offs, *_ = CC.components_host(bad, offs, hs, ws, 4, CC.ONES, capacity=16, fill=77)
    assert st == SHAPE and msg.startswith("rle_components_host:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg and (comp_offs == 77).all()
    st, msg, *_ = CC.select_host(bad, offs, hs, ws, 4, CC.ONES, np.ones(5, np.uint8), CC.MERGE, capacity=64)
    assert st == SHAPE and msg.startswith("rle_components_select_host:") and "RLE 1 sums to" in msg
    for conn, of, what in ((6, 1, "connectivity 6"), (4, 2, "unknown of 2")):
        st, msg, *_ = CC.components_host(counts, offs, hs, ws, conn, of, capacity=16)
        assert st == SHAPE and what in msg, msg
    st, msg, *_ = CC.components_host(counts, offs, [20, 0, 16], ws, 4, 1, capacity=16)
    assert st == SHAPE and "RLE 1 is 0x5" in msg
    st, msg, *_ = CC.select_host(counts, offs, hs, ws, 4, CC.ZEROS, np.ones(5, np.uint8), CC.SPLIT, capacity=64)
    assert st == SHAPE and "SPLIT" in msg
    st, msg, *_ = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, np.ones(5, np.uint8), 2, capacity=64)
    assert st == SHAPE and "unknown mode 2" in msg
    down = offs.copy(); down[2] = down[1] - 1
    st, msg, *_ = CC.components_host(counts, down, hs, ws, 4, 1, capacity=16)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg


def _host_values(fill=77):
    """the arguments of a good call in host memory, every output pre-filled -> (values, the output arrays)"""
    lib = _mod("_lib")
    _planes, counts, offs, hs, ws = _three()
    (counts, offs, hs, ws), _head = CC._set(counts, offs, hs, ws)
    outs = {"comp_offsets": np.full(4, fill, np.int64), "comp_areas": np.full(8, fill, np.uint32), "comp_bboxes_xywh": np.full((8, 4), fill, np.int32),
            "comp_flags": np.full(8, fill, np.uint8), "out_counts": np.full(512, fill, np.uint32), "out_run_offsets": np.full(6, fill, np.int64),
            "areas": np.full(5, fill, np.uint32), "bboxes_xywh": np.full((5, 4), fill, np.int32), "out_parent": np.full(5, fill, np.int64)}
    out_n = C.c_int64(fill)
    keep = np.ones(5, np.uint8)
    values = {"counts": counts.ctypes.data, "run_offsets": offs.ctypes.data, "n": 3, "heights": hs.ctypes.data, "widths": ws.ctypes.data, "connectivity": 4, "of": 1,
              "memspace": lib.HOST, "keep": keep.ctypes.data, "n_comps": 5, "mode": CC.MERGE, "comp_capacity": 8, "capacity": 512, "out_n": C.byref(out_n),
              **{k: a.ctypes.data for k, a in outs.items()}}
    return values, outs, out_n, (counts, offs, hs, ws, keep)


@pytest.mark.parametrize("host_twin", [True, False])
def test_every_argument_error_is_answered_before_anything_is_written_or_a_device_looked_for(pkg, host_twin):
    """the _host twins, and the device entries in host memory on whatever machine this is: an argument error needs no device"""
    values, outs, out_n, _alive = _host_values()
    for entry, changed, status, word in CC.ARGUMENT_ERRORS:
        if host_twin and "memspace" in changed:
            continue
        st, msg = CC.call_with(entry, values, changed, host_twin)
        who = ("rle_components" if entry == "measure" else "rle_components_select") + ("_host:" if host_twin else ":")
        assert st == status and msg.startswith(who) and word in msg, (entry, changed, st, msg)
        assert all((a == 77).all() for a in outs.values()) and out_n.value == 77, (entry, changed)


def test_the_device_entries_answer_err_hip_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _mod("_lib")
    L = lib.lib()
    _planes, counts, offs, hs, ws = _three()
    (counts, offs, hs, ws), head = CC._set(counts, offs, hs, ws)
    comp_offs = np.full(4, 77, np.int64)
    st = L.mrcnn_rle_components(*head, 4, 1, lib.HOST, comp_offs.ctypes.data, None, None, None, 0)
    assert st == HIP and (comp_offs == 77).all(), L.mrcnn_last_error().decode()
    keep, out_n = np.ones(5, np.uint8), C.c_int64(-1)
    st = L.mrcnn_rle_components_select(*head, 4, 1, keep.ctypes.data, 5, CC.MERGE, lib.HOST, None, 0, comp_offs.ctypes.data, None, None, None, C.byref(out_n))
    assert st == HIP and (comp_offs == 77).all() and out_n.value == -1
    # argument errors come first
    st = L.mrcnn_rle_components(*head, 5, 1, lib.HOST, comp_offs.ctypes.data, None, None, None, 0)
    assert st == SHAPE and L.mrcnn_last_error().decode().startswith("rle_components:")
    st = L.mrcnn_rle_components_select(*head, 4, 0, keep.ctypes.data, 5, CC.SPLIT, lib.HOST, None, 0, comp_offs.ctypes.data, None, None, comp_offs.ctypes.data, C.byref(out_n))
    assert st == SHAPE and L.mrcnn_last_error().decode().startswith("rle_components_select:")
