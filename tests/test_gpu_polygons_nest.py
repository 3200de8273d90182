"""Polygon rings nested on the GPU (mrcnn_polygons_nest; detection.nest_polygons).  Every comparison is bit for bit against the
sequential host definition, which tests/test_polygons_nest_host.py pins against connected components of the decoded planes: parent,
depth, rle_polys, poly_rings, ring_order and n_polys, from host memory and from device tensors.

The cases put hundreds of rings into one RLE (more candidates than a workgroup has waves, more target rings than one block), a ring of
more than 2048 vertices (the lanes wrap over its edges), empty RLEs between full ones and rings without vertices into one call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import nest_cases as NC
import polygons_cases as PC
import unite_cases as UC

pytestmark = pytest.mark.gpu
SHAPE = NC.SHAPE


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _both_memspaces_equal_the_definition(arrays, what):
    """the device entry from host memory and from device tensors against the host entry -> the host's arrays"""
    D = _det()
    flat = {k: arrays[k] for k in ("rle_rings", "ring_offsets", "xy")}
    want = NC.nest_host(arrays)
    got = D.nest_polygons(flat)
    assert isinstance(got["parent"], np.ndarray), what
    NC.assert_same(got, want, f"{what}, host memory:")
    dev = D.nest_polygons({k: _cuda(v) for k, v in flat.items()})
    assert all(dev[k].is_cuda for k in NC.KEYS), what
    NC.assert_same(dev, want, f"{what}, device memory:")
    return want


@pytest.fixture(scope="module")
def traced(pkg):
    cases = NC.all_cases()
    return [n for n, _ in cases], PC.trace_host([r for _, r in cases])


# ---- 1. device against host ------------------------------------------------------------------------------------------------------------
def test_one_ragged_call_over_all_the_cases(traced):
    names, tr = traced
    assert len(names) > 840 and tr["n_rings"] > 3500
    want = _both_memspaces_equal_the_definition(tr, "all cases")
    assert want["depth"].max() == 11 and want["n_polys"] > 3000 and (np.diff(want["rle_polys"]) == 0).any()


@pytest.mark.parametrize("name", ["comb", "checkerboard/40x41", "concentric", "c_shape", "1x1/set"])
def test_single_cases(traced, name):
    names, tr = traced
    k = names.index(name)
    r0, r1 = int(tr["rle_rings"][k]), int(tr["rle_rings"][k + 1])
    ro = tr["ring_offsets"]
    one = {"rle_rings": np.array([0, r1 - r0], np.int64), "ring_offsets": ro[r0:r1 + 1] - ro[r0], "xy": tr["xy"][int(ro[r0]):int(ro[r1])],
           "ring_areas": tr["ring_areas"][r0:r1]}
    want = _both_memspaces_equal_the_definition(one, name)
    NC.assert_invariants(want, one)


def test_a_ragged_set_with_empty_slots(pkg):
    rows, sizes, _planes = NC.ragged_set()
    flat = [r for row in rows for r in row]
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    tr = PC.trace_host(flat, n_images=3, slots=4, hs=hs, ws=ws)
    want = _both_memspaces_equal_the_definition(tr, "ragged")
    assert np.diff(want["rle_polys"]).tolist() == [0, 3, 0, 3, 2, 0, 0, 1, 6, 0, 6, 0]


def test_simplified_and_hand_made_rings(traced):
    _names, tr = traced
    D = _det()
    simple = D.simplify_polygons_host(tr, 2.0)
    assert (np.diff(simple["ring_offsets"]) < 3).any()
    want = _both_memspaces_equal_the_definition(simple, "simplified at 2 px")
    assert (want["parent"] != NC.nest_host(tr)["parent"]).any()                                       # general rings: not the traced nesting again
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    rings = [sq(0, 0, 8, 8), [(0, 0), (0, 8), (8, 8), (8, 0)], [], sq(2, 2, 6, 6), [(3, 3)], [(3, 3), (5, 5)], sq(0, 0, 8, 8), [(1, 1), (7, 1), (1, 7)],
             [(7, 1), (7, 7), (1, 7)], [(3, 4), (4, 4), (4, 5)], sq(0, 0, 32767, 32767), [(1, 32766), (32766, 1), (32766, 32766)], []]
    ro = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    arrays = {"rle_rings": np.array([0, 0, 8, 10, 10, 13], np.int64), "ring_offsets": ro, "xy": np.array([p for r in rings for p in r], np.int32).reshape(-1, 2)}
    want = _both_memspaces_equal_the_definition(arrays, "hand-made")
    assert want["parent"].tolist() == [-1, 0, -1, 7, 3, 3, 0, 0, -1, -1, -1, 10, -1]                 # ties, an empty ring, a probe on an edge, the largest plane


# ---- 2. the device-resident flow -----------------------------------------------------------------------------------------------------
def test_rings_traced_on_the_device_are_nested_where_they_lie(pkg):
    D = _det()
    rows, sizes, _planes = NC.ragged_set()
    flat = D.rle_to_polygons(rows, sizes, device="cuda", flat=True)
    assert flat["xy"].is_cuda and flat["rle_rings"].is_cuda
    got = D.nest_polygons(flat)                                  # tensors in, tensors out
    assert all(got[k].is_cuda for k in NC.KEYS)
    host = D.rle_to_polygons_host(rows, sizes, flat=True)
    NC.assert_same(got, D.nest_polygons_host(host), "device-resident")
    both = D.rle_to_polygons(rows, sizes, device="cuda", flat=True, nest=True, tolerance=1.0)
    assert both["nest"]["parent"].is_cuda and both["xy"].is_cuda and both["n_vertices"] < flat["n_vertices"]
    NC.assert_same(both["nest"], got, "rle_to_polygons(nest=True, tolerance=1)")                      # the TRACED rings' nesting


def test_the_empty_set(pkg):
    import torch
    lib = _lib()
    L = lib.lib()
    D = _det()
    for K in (0, 3):
        got = D.nest_polygons({"rle_rings": np.zeros(K + 1, np.int64), "ring_offsets": np.zeros(1, np.int64), "xy": np.zeros((0, 2), np.int32)})
        assert got["n_polys"] == 0 and got["rle_polys"].tolist() == [0] * (K + 1) and got["poly_rings"].tolist() == [0] and len(got["parent"]) == 0
        rr, ro = torch.zeros(K + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        rle_polys, poly_rings = torch.full((K + 1,), -9, dtype=torch.int64, device="cuda"), torch.full((1,), -9, dtype=torch.int64, device="cuda")
        total = C.c_int64(-9)
        lib.check(L.mrcnn_polygons_nest(rr.data_ptr(), K, ro.data_ptr(), None, 0, lib.DEVICE, None, None, rle_polys.data_ptr(), poly_rings.data_ptr(), None,
                                        C.byref(total)))
        assert total.value == 0 and rle_polys.cpu().tolist() == [0] * (K + 1) and poly_rings.cpu().tolist() == [0]


# ---- 3. a bad array in device memory ---------------------------------------------------------------------------------------------------
def _device_call(rr, ro, xy, fill=-9):
    import torch
    lib = _lib()
    L = lib.lib()
    K, R = len(rr) - 1, len(ro) - 1
    bufs = [torch.full((m,), fill, dtype=dt, device="cuda") for m, dt in ((R, torch.int64), (R, torch.int32), (K + 1, torch.int64), (R + 1, torch.int64),
                                                                          (R, torch.int64))]
    total = C.c_int64(fill)
    rr_g, ro_g, xy_g = _cuda(rr), _cuda(ro), _cuda(xy)
    st = L.mrcnn_polygons_nest(rr_g.data_ptr(), K, ro_g.data_ptr(), xy_g.data_ptr(), R, lib.DEVICE, *(b.data_ptr() for b in bufs), C.byref(total))
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs], total.value


def test_a_bad_array_on_the_device_is_named_and_nothing_is_written(pkg):
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    rings = [sq(0, 0, 9, 9), sq(1, 1, 4, 4)[::-1], sq(20, 0, 25, 5), sq(0, 0, 3, 3)]
    ro = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    rr, xy = np.array([0, 2, 2, 3, 4], np.int64), np.array([p for r in rings for p in r], np.int32).reshape(-1, 2)
    st, msg, bufs, total = _device_call(rr, ro, xy)
    assert st == 0 and total == 3 and bufs[0].tolist() == [-1, 0, -1, -1], msg
    at = int(ro[2]) + 1                                          # a vertex of ring 2
    edit = lambda a, i, v: np.concatenate((a[:i], [v], a[i + 1:])).astype(a.dtype)
    low, high = xy.copy(), xy.copy()
    low[at, 0], high[at, 1] = -1, 32768
    for r_, o_, v_, needle in ((rr, ro, low, "ring 2 has a coordinate outside 0..32767"), (rr, ro, high, "ring 2 has a coordinate outside 0..32767"),
                               (rr, edit(ro, 4, ro[3] - 2), xy, "at ring 3"), (edit(rr, 2, 1), ro, xy, "at RLE 1"), (edit(rr, 4, 3), ro, xy, "at RLE 3")):
        st, msg, bufs, total = _device_call(r_, o_, v_)
        assert st == SHAPE and needle in msg and msg.startswith("polygons_nest:"), (needle, st, msg)
        assert all((b == -9).all() for b in bufs) and total == -9, needle


# ---- 4. the wrappers -------------------------------------------------------------------------------------------------------------------
def test_the_rings_of_unite_tiles_come_with_their_nesting(pkg):
    D = _det()
    sc = next(s for s in UC.scenes() if s["name"] == "two_images")
    resident = []
    import tiles_cases as TC
    D._merge_tiles(False, _cuda(sc["det"]), _cuda(sc["masks"]), sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, sc["max_out"], unite=True,
                   resident=resident)
    counts_g, offs_g = resident[0]
    sizes = [tuple(s) for s in sc["sizes"]]
    flat = D.rle_to_polygons((counts_g, offs_g), sizes, flat=True, nest=True, tolerance=1.0)
    assert flat["nest"]["ring_order"].is_cuda
    plain = D.rle_to_polygons_host((counts_g, offs_g), sizes, flat=True)
    want = D.nest_polygons_host(plain)
    NC.assert_same(flat["nest"], want, "unite_tiles")
    assert want["n_polys"] >= 2


def test_predict_tiled_returns_the_nesting_of_the_traced_rings(pkg, small_model):
    d, _cfg = small_model
    D = _det()
    m = importlib.import_module("mask-rcnn-coreml_amd.models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25)
    res = m.predict_tiled(images, polygons=True, nest=True, tolerance=1.0, **kw)
    rings, areas, N = res[4]
    traced_rings = D.rle_to_polygons_host(res[3], [(200, 333), (300, 260)])
    want = D.nest_polygons_host(traced_rings)
    assert N["nest"] == want["nest"] and sum(len(g) for row in N["nest"] for rle in row for g in rle) >= 1
    for b in range(2):
        for i in range(6):
            np.testing.assert_array_equal(N["parent"][b][i], want["parent"][b][i])
            np.testing.assert_array_equal(N["depth"][b][i], want["depth"][b][i])
            assert len(rings[b][i]) == len(traced_rings[0][b][i]) == len(N["depth"][b][i])           # it indexes the simplified rings one for one
    G = importlib.import_module("mask-rcnn-coreml_amd.geojson")
    fc = G.feature_collection(res[0], res[4], None, sizes=[(200, 333), (300, 260)])
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) >= 1
