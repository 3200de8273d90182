"""Connected components of run-length masks on the GPU (mrcnn_rle_components, mrcnn_rle_components_select; detection.rle_components
and its helpers; predict_tiled's min_component_area and fill_holes).  Every comparison is bit for bit against the sequential host
definition, which tests/test_rle_components_host.py pins against a pixel union-find on dense planes: every output array, from host
memory and from device tensors.

The cases (tests/components_cases.py) make long chains (spirals), late merges (U shapes), thousands of one-pixel components
(checkerboards), pieces that join across column ends, single-row planes, zero-length runs and piece counts around
components_cases.PIECES_THRESHOLD; one 2100x2100 plane puts a million pieces into one call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import components_cases as CC
import morph_cases as MC
import unite_cases as UC

pytestmark = pytest.mark.gpu
SHAPE, INVALID = CC.SHAPE, CC.INVALID
MEASURES = ("comp_offsets", "comp_areas", "comp_bboxes_xywh", "comp_flags")
SELECTED = ("out_counts", "out_run_offsets", "areas", "bboxes_xywh", "out_parent")


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _cuda(x):
    import torch
    a = np.ascontiguousarray(x)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _sizes(hs, ws):
    return list(zip(np.asarray(hs).tolist(), np.asarray(ws).tolist()))


def _measures_in_both_memspaces(counts, offs, hs, ws, conn, of, what):
    """the device entry from host memory and from device tensors against the host entry -> the host's four arrays"""
    D = _mod("detection")
    sizes = _sizes(hs, ws)
    want = D.rle_components_host((counts, offs), sizes, conn, of)
    got = D.rle_components((counts, offs), sizes, conn, of)
    assert isinstance(got[1], np.ndarray), what
    CC.assert_same(got, want, MEASURES, f"{what}, host memory")
    dev = D.rle_components((_cuda(counts), _cuda(offs)), sizes, conn, of)
    assert all(a.is_cuda for a in dev), what
    CC.assert_same(dev, want, MEASURES, f"{what}, device memory")
    return want


def _flatten(sel):
    """((counts, run_offsets), areas, bboxes[, parent]) as five arrays (MERGE has no parent: its offsets stand in)"""
    return (sel[0][0], sel[0][1], sel[1], sel[2], sel[3] if len(sel) > 3 else sel[0][1])


def _selection_in_both_memspaces(counts, offs, hs, ws, conn, of, keep, mode, what):
    D = _mod("detection")
    sizes = _sizes(hs, ws)
    want = _flatten(D.rle_select_components_host((counts, offs), sizes, keep, conn, of, mode))
    got = _flatten(D.rle_select_components((counts, offs), sizes, keep, conn, of, mode))
    assert isinstance(got[0], np.ndarray), what
    CC.assert_same(got, want, SELECTED, f"{what}, host memory")
    dev = _flatten(D.rle_select_components((_cuda(counts), _cuda(offs)), sizes, _cuda(keep), conn, of, mode))
    assert all(a.is_cuda for a in dev), what
    CC.assert_same(dev, want, SELECTED, f"{what}, device memory")
    return want


@pytest.fixture(scope="module")
def cases(pkg):
    return CC.all_cases()


# ---- 1. device against host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("of,conn", CC.COMBOS)
def test_one_ragged_call_over_all_the_cases(cases, of, conn):
    assert len(cases) > 500
    counts, offs, hs, ws = CC.flat_set(cases)
    want = _measures_in_both_memspaces(counts, offs, hs, ws, conn, of, f"all cases, of {of}, connectivity {conn}")
    comp_offs, areas, _boxes, flags = want
    assert (np.diff(comp_offs) == 0).any() and (np.diff(comp_offs) > 1000).any() and (flags == 0).any() and (flags == 1).any()
    D = _mod("detection")
    again = D.rle_components((_cuda(counts), _cuda(offs)), _sizes(hs, ws), conn, of)                # the same call twice is bit-equal
    CC.assert_same(again, want, MEASURES, "the second call")

    # MERGE (and SPLIT of ones) with the keep masks the helpers build, and with a seeded random one
    a = areas.astype(np.int64)
    rng = np.random.default_rng(8)
    masks = {"helper": a >= 5 if of == CC.ONES else ((flags & 1) != 0) | (a > 3), "random": rng.random(len(a)) < 0.5}
    if (of, conn) == (CC.ONES, 4):
        masks["largest"] = D._largest_mask(comp_offs, a, 1)
    for name, keep in masks.items():
        keep = np.ascontiguousarray(keep, np.uint8)
        what = f"all cases, of {of}, connectivity {conn}, keep {name}"
        first = _selection_in_both_memspaces(counts, offs, hs, ws, conn, of, keep, "merge", what + ", merge")
        if of == CC.ONES and name != "largest":
            _selection_in_both_memspaces(counts, offs, hs, ws, conn, of, keep, "split", what + ", split")
        if name == "random":
            second = _flatten(D.rle_select_components((_cuda(counts), _cuda(offs)), _sizes(hs, ws), _cuda(keep), conn, of, "merge"))
            CC.assert_same(second, first, SELECTED, "the second selection")


SINGLES = ["one_by_one_set", "one_by_one_clear", "row_run_over_five_columns", "column_two_pieces/zero_runs", "diagonal_pair", "antidiagonal_pair",
           "diagonal_line", "u", "inverted_u", "spiral_33", "two_spirals_41", "rings_21", "checkerboard_64", "bottom_beside_top", "bottom_beside_top_two_rows",
           "zeros_bottom_beside_top", "row_alternating", "comb/130x130", "empty/5x5", "full/5x5", "full/1x7", "pinholes_specks/300x260", "random_0.6",
           f"pieces_{CC.PIECES_THRESHOLD - 1}", f"pieces_{CC.PIECES_THRESHOLD}", f"pieces_{CC.PIECES_THRESHOLD + 1}", f"pieces_{CC.PIECES_THRESHOLD}_inverse"]


@pytest.mark.parametrize("prefix", SINGLES)
def test_single_cases(cases, prefix):
    name, counts, h, w, _plane = next(c for c in cases if c[0].startswith(prefix))
    offs = np.array([0, len(counts)], np.int64)
    for of, conn in CC.COMBOS:
        want = _measures_in_both_memspaces(counts, offs, [h], [w], conn, of, f"{name}, of {of}, connectivity {conn}")
        n = len(want[1])
        for which, keep in (("all", np.ones(n, np.uint8)), ("none", np.zeros(n, np.uint8)), ("odd", (np.arange(n) & 1).astype(np.uint8))):
            _selection_in_both_memspaces(counts, offs, [h], [w], conn, of, keep, "merge", f"{name}, of {of}, connectivity {conn}, merge {which}")
            if of == CC.ONES:
                _selection_in_both_memspaces(counts, offs, [h], [w], conn, of, keep, "split", f"{name}, connectivity {conn}, split {which}")


def test_the_large_case(pkg):
    D = _mod("detection")
    P, spiral_area = CC.large_case()
    counts = MC.encode(P)
    pair, sizes = (counts, np.array([0, len(counts)], np.int64)), [(2100, 2100)]
    want = D.rle_components_host(pair, sizes, 4, "ones")
    got = D.rle_components((_cuda(pair[0]), _cuda(pair[1])), sizes, 4, "ones")
    CC.assert_same(got, want, MEASURES, "2100x2100")
    assert int(want[1][0]) == spiral_area and want[2][0].tolist() == [0, 0, 1400, 1400] and len(want[1]) > 30000      # the spiral is one component
    keep = (want[1] >= 2).astype(np.uint8)
    merged = _flatten(D.rle_select_components((_cuda(pair[0]), _cuda(pair[1])), sizes, _cuda(keep), 4, "ones", "merge"))
    CC.assert_same(merged, _flatten(D.rle_select_components_host(pair, sizes, keep, 4, "ones", "merge")), SELECTED, "2100x2100, merge")
    keep = (want[1] >= 3).astype(np.uint8)                           # SPLIT sorts a million pieces: the grid-wide steps of the network
    cut = _flatten(D.rle_select_components((_cuda(pair[0]), _cuda(pair[1])), sizes, _cuda(keep), 4, "ones", "split"))
    CC.assert_same(cut, _flatten(D.rle_select_components_host(pair, sizes, keep, 4, "ones", "split")), SELECTED, "2100x2100, split")


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------------------
def _three():
    planes = [MC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), CC.rings(16)]
    runs = [MC.encode(p) for p in planes]
    return planes, np.concatenate(runs), np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64), [20, 7, 16], [30, 5, 16]


def _device_measures(counts, offs, hs, ws, conn, of, capacity, fill=77, arrays=True):
    """mrcnn_rle_components on device tensors with pre-filled outputs -> (status, message, [comp_offsets, areas, bboxes, flags])"""
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n = len(offs) - 1
    c_g, o_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64))
    hs, ws = (np.ascontiguousarray(a, np.int32) for a in (hs, ws))
    cap = max(1, capacity)
    bufs = [torch.full((n + 1,), fill, dtype=torch.int64, device="cuda"), torch.full((cap,), fill, dtype=torch.int32, device="cuda"),
            torch.full((cap, 4), fill, dtype=torch.int32, device="cuda"), torch.full((cap,), fill, dtype=torch.uint8, device="cuda")]
    ptrs = [b.data_ptr() if arrays or i == 0 else None for i, b in enumerate(bufs)]
    st = L.mrcnn_rle_components(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, conn, of, lib.DEVICE, *ptrs, capacity if arrays else 0)
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs]


def _device_select(counts, offs, hs, ws, conn, of, keep, mode, capacity, fill=77, out=True, n_comps=None):
    """mrcnn_rle_components_select on device tensors with pre-filled outputs -> (status, message, [out_counts, out_run_offsets, areas,
    bboxes, out_parent], out_n)"""
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n = len(offs) - 1
    c_g, o_g, k_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64)), _cuda(np.ascontiguousarray(keep, np.uint8))
    hs, ws = (np.ascontiguousarray(a, np.int32) for a in (hs, ws))
    room = max(n, len(keep)) + 1
    bufs = [torch.full((max(1, capacity),), fill, dtype=torch.int32, device="cuda"), torch.full((room,), fill, dtype=torch.int64, device="cuda"),
            torch.full((room,), fill, dtype=torch.int32, device="cuda"), torch.full((room, 4), fill, dtype=torch.int32, device="cuda"),
            torch.full((room,), fill, dtype=torch.int64, device="cuda")]
    out_n = C.c_int64(fill)
    st = L.mrcnn_rle_components_select(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, conn, of, k_g.data_ptr(),
                                       len(keep) if n_comps is None else n_comps, mode, lib.DEVICE, bufs[0].data_ptr() if out else None,
                                       capacity if out else 0, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), C.byref(out_n))
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs], int(out_n.value)


def test_argument_errors_leave_the_outputs_alone(pkg):
    _planes, counts, offs, hs, ws = _three()
    for conn, of, text in ((6, 1, "connectivity 6 is neither 4 nor 8"), (4, 2, "unknown of 2")):
        st, msg, bufs = _device_measures(counts, offs, hs, ws, conn, of, 16)
        assert st == SHAPE and msg.startswith("rle_components:") and text in msg, msg
        assert all((b == 77).all() for b in bufs)
    st, msg, bufs = _device_measures(counts, offs, [20, 40000, 16], ws, 4, 1, 16)
    assert st == SHAPE and "RLE 1 is 40000x5" in msg and all((b == 77).all() for b in bufs)
    keep = np.ones(5, np.uint8)
    for of, mode, text in ((CC.ZEROS, CC.SPLIT, "SPLIT"), (CC.ONES, 2, "unknown mode 2")):
        st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, of, keep, mode, 64)
        assert st == SHAPE and msg.startswith("rle_components_select:") and text in msg, msg
        assert all((b == 77).all() for b in bufs) and out_n == 77
    lib = _mod("_lib")
    c_g, o_g = _cuda(counts), _cuda(offs)
    h32, w32 = np.asarray(hs, np.int32), np.asarray(ws, np.int32)
    assert lib.lib().mrcnn_rle_components(c_g.data_ptr(), o_g.data_ptr(), 3, h32.ctypes.data, w32.ctypes.data, 4, 1, 7, o_g.data_ptr(), None, None, None, 0) == INVALID
    assert "unknown memspace 7" in lib.lib().mrcnn_last_error().decode()
    assert lib.lib().mrcnn_rle_components(c_g.data_ptr(), o_g.data_ptr(), 3, h32.ctypes.data, w32.ctypes.data, 4, 1, lib.DEVICE, None, None, None, None, 0) == INVALID


def test_every_argument_error_on_device_tensors_leaves_them_alone(pkg):
    import torch
    lib = _mod("_lib")
    _planes, counts, offs, hs, ws = _three()
    c_g, o_g, k_g = _cuda(counts), _cuda(offs), _cuda(np.ones(5, np.uint8))
    h32, w32 = np.asarray(hs, np.int32), np.asarray(ws, np.int32)
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device="cuda")
    outs = {"comp_offsets": full((4,), torch.int64), "comp_areas": full((8,), torch.int32), "comp_bboxes_xywh": full((8, 4), torch.int32),
            "comp_flags": full((8,), torch.uint8), "out_counts": full((512,), torch.int32), "out_run_offsets": full((6,), torch.int64),
            "areas": full((5,), torch.int32), "bboxes_xywh": full((5, 4), torch.int32), "out_parent": full((5,), torch.int64)}
    out_n = C.c_int64(77)
    values = {"counts": c_g.data_ptr(), "run_offsets": o_g.data_ptr(), "n": 3, "heights": h32.ctypes.data, "widths": w32.ctypes.data, "connectivity": 4, "of": 1,
              "memspace": lib.DEVICE, "keep": k_g.data_ptr(), "n_comps": 5, "mode": CC.MERGE, "comp_capacity": 8, "capacity": 512, "out_n": C.byref(out_n),
              **{k: a.data_ptr() for k, a in outs.items()}}
    assert CC.call_with("measure", values, {})[0] == 0 and CC.call_with("select", values, {})[0] == 0 and out_n.value == 3      # the good call is good
    for a in outs.values():
        a.fill_(77)
    out_n.value = 77
    for entry, changed, status, word in CC.ARGUMENT_ERRORS:
        st, msg = CC.call_with(entry, values, changed)
        torch.cuda.synchronize()
        assert st == status and msg.startswith("rle_components:" if entry == "measure" else "rle_components_select:") and word in msg, (entry, changed, st, msg)
        assert all(bool((a == 77).all()) for a in outs.values()) and out_n.value == 77, (entry, changed)


def test_a_bad_total_on_the_device_is_named_and_nothing_is_written(pkg):
    _planes, counts, offs, hs, ws = _three()
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1, and RLE 2 as well: the lowest is named
    bad[int(offs[2])] += 1
    for of in (CC.ONES, CC.ZEROS):
        st, msg, bufs = _device_measures(bad, offs, hs, ws, 4, of, 16)
        assert st == SHAPE and msg.startswith("rle_components:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg, msg
        assert all((b == 77).all() for b in bufs)
        st, msg, bufs, out_n = _device_select(bad, offs, hs, ws, 4, of, np.ones(5, np.uint8), CC.MERGE, 64)
        assert st == SHAPE and msg.startswith("rle_components_select:") and "RLE 1 sums to 38 pixels" in msg, msg
        assert all((b == 77).all() for b in bufs) and out_n == 77
    down = offs.copy()
    down[2] = down[1] - 1
    st, msg, bufs = _device_measures(counts, down, hs, ws, 4, 1, 16)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg and all((b == 77).all() for b in bufs)


def test_the_component_capacity_and_its_size_query(pkg):
    _planes, counts, offs, hs, ws = _three()
    st, msg, bufs = _device_measures(counts, offs, hs, ws, 4, CC.ONES, 0, arrays=False)               # capacity 0, null arrays
    assert st == SHAPE and msg.startswith("rle_components:") and "comp_capacity >= 5" in msg, msg
    assert bufs[0].tolist() == [0, 1, 2, 5] and all((b == 77).all() for b in bufs[1:])
    st, msg, bufs = _device_measures(counts, offs, hs, ws, 4, CC.ONES, 4)
    assert st == SHAPE and "comp_capacity >= 5" in msg and bufs[0].tolist() == [0, 1, 2, 5] and all((b == 77).all() for b in bufs[1:])
    st, msg, bufs = _device_measures(counts, offs, hs, ws, 4, CC.ONES, 8)
    st_h, _m, offs_h, areas_h, boxes_h, flags_h = CC.components_host(counts, offs, hs, ws, 4, CC.ONES)
    assert st == 0 and st_h == 0 and bufs[0].tolist() == offs_h.tolist() and bufs[1][:5].view(np.uint32).tolist() == areas_h.tolist()
    assert (bufs[2][:5] == boxes_h).all() and bufs[3][:5].tolist() == flags_h.tolist() == [0, 1, 1, 0, 0]
    assert (bufs[1][5:] == 77).all() and (bufs[2][5:] == 77).all() and (bufs[3][5:] == 77).all()
    st, msg, bufs = _device_measures(np.zeros(1, np.uint32), np.zeros(1, np.int64), [], [], 4, CC.ONES, 4)                       # n = 0
    assert st == 0 and bufs[0].tolist() == [0], msg


def test_the_selection_capacity_its_size_query_and_n_comps(pkg):
    _planes, counts, offs, hs, ws = _three()
    keep = np.array([1, 1, 0, 1, 1], np.uint8)
    for mode, n_out in ((CC.MERGE, 3), (CC.SPLIT, 4)):
        want = CC.select_host(counts, offs, hs, ws, 4, CC.ONES, keep, mode)
        assert want[0] == 0 and len(want[6]) == n_out
        need = len(want[2])
        st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, CC.ONES, keep, mode, 0, out=False)         # capacity 0, out_counts NULL
        assert st == SHAPE and msg.startswith("rle_components_select:") and f"capacity >= {need}" in msg, msg
        assert out_n == n_out and bufs[1][:n_out + 1].tolist() == want[3].tolist() and bufs[2][:n_out].view(np.uint32).tolist() == want[4].tolist()
        assert (bufs[3][:n_out] == want[5]).all() and bufs[4][:n_out].tolist() == want[6].tolist() and (bufs[1][n_out + 1:] == 77).all()
        st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, CC.ONES, keep, mode, need - 1)
        assert st == SHAPE and f"capacity >= {need}" in msg and (bufs[0] == 77).all() and bufs[1][:n_out + 1].tolist() == want[3].tolist()
        st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, CC.ONES, keep, mode, need + 5)
        assert st == 0 and bufs[0][:need].view(np.uint32).tolist() == want[2].tolist() and (bufs[0][need:] == 77).all() and out_n == n_out
        for wrong in (4, 6):
            st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, CC.ONES, keep, mode, 64, n_comps=wrong)
            assert st == SHAPE and f"n_comps = {wrong}" in msg and "5 components" in msg, msg
            assert all((b == 77).all() for b in bufs) and out_n == 77
    st, msg, bufs, out_n = _device_select(np.zeros(1, np.uint32), np.zeros(1, np.int64), [], [], 4, CC.ONES, np.zeros(0, np.uint8), CC.MERGE, 4)      # n = 0
    assert st == 0 and out_n == 0 and bufs[1][0] == 0, msg
    st, msg, bufs, out_n = _device_select(counts, offs, hs, ws, 4, CC.ONES, np.zeros(5, np.uint8), CC.SPLIT, 4)                  # nothing kept
    assert st == 0 and out_n == 0 and bufs[1][0] == 0, msg


def test_a_split_past_the_first_guess_takes_the_wrappers_second_attempt(pkg, monkeypatch):
    """the top and the bottom row of a 3 x 8 plane (tests/test_rle_components_host.py says why): 18 runs and two components, a first
    guess of 18 + 2 * 2 + 2 = 24 and a result of 33 runs, from host memory and from device tensors"""
    L = _mod("_lib").lib()
    plane = np.zeros((3, 8), np.uint8)
    plane[[0, 2]] = 1
    runs = MC.encode(plane)
    entry, capacities = L.mrcnn_rle_components_select, []
    monkeypatch.setattr(L, "mrcnn_rle_components_select", lambda *a: capacities.append(a[12]) or entry(*a))
    want = _selection_in_both_memspaces(runs, np.array([0, 18], np.int64), [3], [8], 4, "ones", np.ones(2, np.uint8), "split", "two rows, split")
    assert capacities == [24, 33, 24, 33]                        # from host memory, then from device tensors
    assert want[1].tolist() == [0, 17, 33] and want[4].tolist() == [0, 0]


# ---- 3. the helpers on a resident pair -----------------------------------------------------------------------------------------------------
def test_the_helpers_change_a_resident_pair_where_it_lies(pkg):
    import tiles_cases as TC
    D = _mod("detection")
    sc = next(s for s in UC.scenes() if s["name"] == "two_images")
    resident = []
    D._merge_tiles(False, _cuda(sc["det"]), _cuda(sc["masks"]), sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, sc["max_out"], unite=True,
                   resident=resident)
    sizes = [tuple(s) for s in sc["sizes"]]
    slots = int(sc["max_out"])
    pair_g = (resident[0][0], resident[0][1][:len(sizes) * slots + 1].contiguous())
    pair_h = (pair_g[0].cpu().numpy().view(np.uint32), pair_g[1].cpu().numpy())
    got = D.rle_components(pair_g, sizes)
    assert all(a.is_cuda for a in got)
    CC.assert_same(got, D.rle_components_host(pair_h, sizes), MEASURES, "resident, rle_components")
    assert int(got[0][-1]) > 0
    for name, args in (("rle_remove_small", (40,)), ("rle_keep_largest", (1,)), ("rle_fill_holes", ()), ("rle_fill_holes", (6,))):
        out = getattr(D, name)(pair_g, sizes, *args)
        want = getattr(D, name + "_host")(pair_h, sizes, *args)
        assert out[0].is_cuda and out[1].is_cuda, name
        CC.assert_same(out, want, ("counts", "run_offsets"), f"resident, {name}{args}")
        rings = D.rle_to_polygons(out, sizes, flat=True)                                             # the result feeds the entries after it
        rings_h = D.rle_to_polygons_host(want, sizes, flat=True)
        assert rings["xy"].is_cuda and all((rings[k].cpu().numpy() == rings_h[k]).all() for k in ("rle_rings", "ring_offsets", "ring_areas", "xy"))
    (cut, parent), (cut_h, parent_h) = D.rle_split_components(pair_g, sizes, 10, 8), D.rle_split_components_host(pair_h, sizes, 10, 8)
    assert cut[0].is_cuda and parent.is_cuda
    CC.assert_same((cut[0], cut[1], parent), (cut_h[0], cut_h[1], parent_h), ("counts", "run_offsets", "parent"), "resident, rle_split_components")
    rows = D.rle_rows_of(pair_h, sizes)                          # rows in, rows out, through the device entries
    r_rows, r_areas, r_boxes = D.rle_select_components(rows, None, np.ones(int(got[0][-1]), np.uint8))
    assert r_areas.shape == (len(sizes), slots) and r_boxes.shape == (len(sizes), slots, 4)
    canonical = D.rle_select_components_host(rows, None, np.ones(int(got[0][-1]), np.uint8))[0]
    assert all(r_rows[b][i]["counts"].tolist() == canonical[b][i]["counts"].tolist() for b in range(len(sizes)) for i in range(slots))


# ---- 4. predict_tiled(min_component_area=, fill_holes=) ---------------------------------------------------------------------------------------
def test_predict_tiled_filters_the_kept_masks_by_their_components(pkg, small_model):
    d, _cfg = small_model
    D = _mod("detection")
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    sizes = [(200, 333), (300, 260)]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25, polygons=True)
    plain = m.predict_tiled(images, **kw)
    for nothing in (False, 0, None):                             # the defaults change nothing, and 0 pixels fill nothing
        same = m.predict_tiled(images, min_component_area=0, fill_holes=nothing, **kw)
        for b in range(2):
            for i in range(6):
                assert same[3][b][i]["counts"].tolist() == plain[3][b][i]["counts"].tolist()
    for fill, area in ((True, 30), (12, 0), (False, 50)):
        got = m.predict_tiled(images, min_component_area=area, fill_holes=fill, **kw)
        want = plain[3]
        if fill is not False:                                    # holes first, then specks
            want = D.rle_fill_holes_host(want, sizes, max_area=None if fill is True else fill)
        if area:
            want = D.rle_remove_small_host(want, sizes, area)
        assert sum(int(e["counts"][1::2].sum()) for row in want for e in row) > 0
        for b in range(2):
            for i in range(6):
                assert got[3][b][i]["size"] == want[b][i]["size"] and got[3][b][i]["counts"].tolist() == want[b][i]["counts"].tolist(), (fill, area, b, i)
        for k in range(3):
            assert (np.asarray(got[k]) == np.asarray(plain[k])).all()
        rings_h, _areas_h = D.rle_to_polygons_host(want, sizes)
        for b in range(2):
            for i in range(6):
                assert len(got[4][0][b][i]) == len(rings_h[b][i]) and all((p == q).all() for p, q in zip(got[4][0][b][i], rings_h[b][i]))
