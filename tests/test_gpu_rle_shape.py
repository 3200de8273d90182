"""Measuring run-length masks on the GPU (mrcnn_rle_measure, mrcnn_rle_convex_hull; detection.rle_measure, rle_convex_hull,
rle_region_props; predict_tiled(props=True)).  Every comparison is bit for bit against the sequential host definitions, which
tests/test_rle_shape_host.py pins against numpy and Python-int restatements on dense planes: measures, hull_offsets, xy, hull_areas2
and obb, from host memory and from device tensors.

The cases (tests/shape_cases.py) put all plane sizes into one call, wrap runs over column ends, line candidates up on diagonals and
leave columns empty inside a mask; the other tests stand on both sides of MRCNN_HULL_LDS_COLUMNS, build a hull of hundreds of vertices
in global scratch, and sum full planes up to 32767 x 32767, where a run spans every column and the moments reach 2^59."""
import importlib

import numpy as np
import pytest

import shape_cases as SC
from test_gpu_rle_morph import _cuda

pytestmark = pytest.mark.gpu
SHAPE = SC.SHAPE


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _measure(host_definition, device, counts, offs, hs, ws):
    D, M = _mod("detection"), _mod("_marshal")
    return D._measure_flat(host_definition, M.Space(device), counts, offs, _i32(hs), _i32(ws))


def _hull(host_definition, device, counts, offs, hs, ws):
    D, M = _mod("detection"), _mod("_marshal")
    return D._hull_flat(host_definition, M.Space(device), counts, offs, _i32(hs), _i32(ws))


def _same(got, want, what):
    host = lambda a: a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    for name, g, w in zip(("hull_offsets", "xy", "hull_areas2", "obb"), got, want):
        g, w = host(g), host(w)
        assert g.shape == w.shape and (g == w).all(), f"{what}: {name} differs" + (f" first at {int(np.flatnonzero((g != w).reshape(-1))[0])}"
                                                                                      if g.shape == w.shape else f": shapes {g.shape} / {w.shape}")


def _both_memspaces_equal_the_definition(runs, hs, ws, what):
    """both device entries from host memory and from device tensors against the host entries -> the host's (measures, hull tables)"""
    counts, offs = SC.flat_set(runs)
    want_m, want_h = _measure(True, None, counts, offs, hs, ws), _hull(True, None, counts, offs, hs, ws)
    got_m, got_h = _measure(False, None, counts, offs, hs, ws), _hull(False, None, counts, offs, hs, ws)
    assert isinstance(got_m, np.ndarray) and isinstance(got_h[1], np.ndarray), what
    assert (got_m == want_m).all(), f"{what}, host memory: measures differ first at RLE {int(np.flatnonzero((got_m != want_m).any(axis=1))[0])}"
    _same(got_h, want_h, f"{what}, host memory")
    c_g, o_g = _cuda(counts), _cuda(offs)
    dev_m, dev_h = _measure(False, "cuda", c_g, o_g, hs, ws), _hull(False, "cuda", c_g, o_g, hs, ws)
    assert dev_m.is_cuda and all(a.is_cuda for a in dev_h), what
    assert (dev_m.cpu().numpy() == want_m).all(), f"{what}, device memory: measures differ"
    _same(dev_h, want_h, f"{what}, device memory")
    return want_m, want_h


# ---- 1. device against host --------------------------------------------------------------------------------------------------------------
def test_one_ragged_call_over_all_the_cases(pkg):
    cases = SC.all_cases()
    assert len(cases["runs"]) == len(SC.SIZES) * len(SC.CONTENTS)
    m, h = _both_memspaces_equal_the_definition(cases["runs"], cases["hs"], cases["ws"], "all cases")
    assert (m[:, 0] == 0).any() and (np.diff(h[0]) == 0).any() and (np.diff(h[0]) > 8).any()


@pytest.mark.parametrize("content", ["sparse", "arch"])
def test_both_sides_of_the_lds_boundary(pkg, content):
    """3 rows and LDS - 2, LDS - 1 and LDS pixel columns: vertex columns one below, at and one above MRCNN_HULL_LDS_COLUMNS"""
    limit = _mod("detection").HULL_LDS_COLUMNS
    rng = np.random.default_rng(5)
    planes = []
    for w in (limit - 2, limit - 1, limit):
        P = (rng.random((3, w)) < 0.01).astype(np.uint8) if content == "sparse" else SC.arch(3, w)
        if content == "sparse":
            P[1, 0] = P[2, w - 1] = 1                            # the hull spans every vertex column
        planes.append(P)
    runs = [SC.encode(P) for P in planes]
    _m, h = _both_memspaces_equal_the_definition(runs, [3] * 3, [p.shape[1] for p in planes], f"LDS boundary, {content}")
    assert (np.diff(h[0]) >= 4).all()
    ring = [tuple(p) for p in h[1][int(h[0][2]):int(h[0][3])].tolist()]                                  # the one in global scratch, against the rule
    assert ring == SC.hull_of(planes[2], columns_only=True)


def test_a_disc_wider_than_the_lds_path(pkg):
    limit = _mod("detection").HULL_LDS_COLUMNS
    radius = limit // 2 + 20
    side = 2 * radius + 3
    assert side + 1 > limit
    P = SC.disc(side, radius)
    m, h = _both_memspaces_equal_the_definition([SC.encode(P)], [side], [side], "disc")
    assert int(h[0][1]) > 200                                    # hundreds of hull vertices
    assert [tuple(p) for p in h[1].tolist()] == SC.hull_of(P, columns_only=True)
    assert int(m[0, 0]) == int(P.sum()) and 2 * int(m[0, 0]) <= int(h[2][0])


def test_full_planes_in_closed_form(pkg):
    """one run that spans every column: the O(1) block of full columns, and the int64 range at 32767 x 32767"""
    sizes = [(32767, 257), (257, 32767)]
    runs = [np.array([0, h * w], np.uint32) for h, w in sizes]
    m, h = _both_memspaces_equal_the_definition(runs, [s[0] for s in sizes], [s[1] for s in sizes], "full planes")
    for k, (hh, ww) in enumerate(sizes):
        assert [int(v) for v in m[k]] == SC.full_measures(hh, ww)
        assert h[1][4 * k:4 * k + 4].tolist() == [[0, 0], [ww, 0], [ww, hh], [0, hh]] and int(h[2][k]) == 2 * hh * ww
    s = 32767
    counts, offs = SC.flat_set([np.array([0, s * s], np.uint32), np.array([s * s], np.uint32)])          # the full plane (two runs) and the empty one
    for device, c, o in ((None, counts, offs), ("cuda", _cuda(counts), _cuda(offs))):
        got = _measure(False, device, c, o, [s, s], [s, s])
        got = got.cpu().numpy() if device else got
        assert [int(v) for v in got[0]] == SC.full_measures(s, s) and int(got[0, 3]) > 2 ** 58 and (got[1] == 0).all()
        ho, xy, a2, obb = (a.cpu().numpy() if device else a for a in _hull(False, device, c, o, [s, s], [s, s]))
        assert ho.tolist() == [0, 4, 4] and xy.tolist() == [[0, 0], [s, 0], [s, s], [0, s]] and a2.tolist() == [2 * s * s, 0]
        assert obb.tolist() == [[0, s, 0, 0, s * s, 0, s * s, 0], [-1, 0, 0, 0, 0, 0, 0, 0]]


# ---- 2. errors and the capacity protocol -------------------------------------------------------------------------------------------------
def _device_hull(counts, offs, hs, ws, capacity, fill=77, out=True):
    """mrcnn_rle_convex_hull on device tensors with pre-filled outputs -> (status, message, n_vertices, [hull_offsets, areas2, obb, xy])"""
    import ctypes as C
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n = len(offs) - 1
    c_g, o_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64))
    hs, ws = _i32(hs), _i32(ws)
    bufs = [torch.full((n + 1,), fill, dtype=torch.int64, device="cuda"), torch.full((max(1, n),), fill, dtype=torch.int64, device="cuda"),
            torch.full((max(1, n), 8), fill, dtype=torch.int64, device="cuda"), torch.full((max(1, capacity), 2), fill, dtype=torch.int32, device="cuda")]
    nv = C.c_int64(fill)
    st = L.mrcnn_rle_convex_hull(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, lib.DEVICE, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                 bufs[2].data_ptr(), bufs[3].data_ptr() if out else None, C.byref(nv), capacity if out else 0)
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), int(nv.value), [b.cpu().numpy() for b in bufs]


def _device_measure(counts, offs, hs, ws, fill=77):
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n = len(offs) - 1
    c_g, o_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64))
    hs, ws = _i32(hs), _i32(ws)
    out = torch.full((max(1, n), 7), fill, dtype=torch.int64, device="cuda")
    st = L.mrcnn_rle_measure(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, lib.DEVICE, out.data_ptr())
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), out.cpu().numpy()


def _four():
    planes = [SC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), SC.ellipse(20, 30, 12, 12, 5, 5), SC.ellipse(7, 5, 3, 2, 2, 1)]
    runs = [SC.encode(p) for p in planes]
    return planes, *SC.flat_set(runs), [20, 7, 20, 7], [30, 5, 30, 5]


def test_a_bad_total_on_the_device_is_named_and_nothing_is_written(pkg):
    planes, counts, offs, hs, ws = _four()
    st, msg, out = _device_measure(counts, offs, hs, ws)
    assert st == 0 and out[:, 0].tolist() == [int(p.sum()) for p in planes], msg
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1, and RLE 3 as well: the lowest is named
    bad[int(offs[3])] -= 1
    st, msg, out = _device_measure(bad, offs, hs, ws)
    assert st == SHAPE and msg.startswith("rle_measure:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg, msg
    assert (out == 77).all()
    st, msg, nv, bufs = _device_hull(bad, offs, hs, ws, 128)
    assert st == SHAPE and msg.startswith("rle_convex_hull:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg, msg
    assert nv == 77 and all((b == 77).all() for b in bufs)
    down = offs.copy()
    down[2] = down[1] - 1
    st, msg, out = _device_measure(counts, down, hs, ws)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg and (out == 77).all()
    st, msg, nv, bufs = _device_hull(counts, down, hs, ws, 128)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg and all((b == 77).all() for b in bufs)


def test_the_size_query_and_a_small_capacity_on_the_device(pkg):
    _planes, counts, offs, hs, ws = _four()
    want = _hull(True, None, counts, offs, hs, ws)
    need = int(want[0][4])
    st, msg, nv, bufs = _device_hull(counts, offs, hs, ws, 0, out=False)                                 # capacity 0, xy NULL
    assert st == SHAPE and f"vertex_capacity >= {need}" in msg and msg.startswith("rle_convex_hull:") and nv == need
    assert bufs[0].tolist() == want[0].tolist() and bufs[1].tolist() == want[2].tolist() and (bufs[2] == want[3]).all()
    st, msg, nv, bufs = _device_hull(counts, offs, hs, ws, need - 1)
    assert st == SHAPE and f"vertex_capacity >= {need}" in msg and (bufs[3] == 77).all() and bufs[0].tolist() == want[0].tolist() and (bufs[2] == want[3]).all()
    st, msg, nv, bufs = _device_hull(counts, offs, hs, ws, need + 5)
    assert st == 0 and nv == need and (bufs[3][:need] == want[1]).all() and (bufs[3][need:] == 77).all()
    import ctypes as C
    import torch
    lib = _mod("_lib")
    o = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    nv = C.c_int64(77)
    assert lib.lib().mrcnn_rle_convex_hull(None, z.data_ptr(), 0, None, None, lib.DEVICE, o.data_ptr(), None, None, None, C.byref(nv), 0) == 0     # n = 0
    assert o.cpu().tolist() == [0] and nv.value == 0
    assert lib.lib().mrcnn_rle_measure(None, z.data_ptr(), 0, None, None, lib.DEVICE, None) == 0


# ---- 3. resident flows -------------------------------------------------------------------------------------------------------------------
def test_components_are_measured_without_leaving_the_device(pkg):
    """rle_split_components -> rle_measure and rle_convex_hull on the resident pair: the parts' moments sum to the whole's"""
    D = _mod("detection")
    cases = SC.all_cases()
    pick = [k for k, name in enumerate(cases["names"]) if name.split("/")[1] in ("33x65", "64x32") and name.split("/")[0] in ("rand05", "gap", "cross", "corners")]
    runs, hs, ws = [cases["runs"][k] for k in pick], cases["hs"][pick], cases["ws"][pick]
    sizes = list(zip(hs.tolist(), ws.tolist()))
    counts, offs = SC.flat_set(runs)
    pair_g = (_cuda(counts), _cuda(offs))
    parts_g, parent_g = D.rle_split_components(pair_g, sizes)
    assert parts_g[0].is_cuda and parent_g.is_cuda
    parent = parent_g.cpu().numpy()
    part_sizes = [sizes[int(p)] for p in parent]
    got = D.rle_measure(parts_g, part_sizes)
    assert got.is_cuda
    parts_h = (parts_g[0].cpu().numpy().view(np.uint32), parts_g[1].cpu().numpy())
    assert (got.cpu().numpy() == D.rle_measure_host(parts_h, part_sizes)).all()
    whole = D.rle_measure(pair_g, sizes).cpu().numpy()
    summed = np.zeros_like(whole)
    np.add.at(summed, parent, got.cpu().numpy())
    assert (summed[:, :6] == whole[:, :6]).all() and (summed[:, 6] == whole[:, 6]).all()         # (4-connected parts share no edge either)
    hull_g = D.rle_convex_hull(parts_g, part_sizes, flat=True)
    assert all(a.is_cuda for a in hull_g)
    _same(hull_g, D.rle_convex_hull_host(parts_h, part_sizes, flat=True), "resident parts")
    props, props_h = D.rle_region_props(parts_g, part_sizes), D.rle_region_props_host(parts_h, part_sizes)
    assert sorted(props) == sorted(D.REGION_PROPS)
    for key in props:
        assert props[key].tobytes() == props_h[key].tobytes(), key


# ---- 4. predict_tiled(props=) --------------------------------------------------------------------------------------------------------------
def test_predict_tiled_appends_the_region_props(pkg, small_model):
    d, _cfg = small_model
    D = _mod("detection")
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    sizes = [(200, 333), (300, 260)]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25, close=1, fill_holes=True, disjoint=True)
    plain = m.predict_tiled(images, **kw)
    with_props = m.predict_tiled(images, props=True, **kw)
    assert len(plain) == 4 and len(with_props) == 5
    for k in range(3):
        assert (np.asarray(with_props[k]) == np.asarray(plain[k])).all()
    want = D.rle_region_props_host(plain[3], sizes)
    assert int(want["area"].sum()) > 0 and want["area"].shape == (12,)
    for key in D.REGION_PROPS:
        assert with_props[4][key].tobytes() == want[key].tobytes(), key
    both = m.predict_tiled(images, props=True, polygons=True, **kw)
    assert len(both) == 6 and both[5]["area"].tolist() == want["area"].tolist()
