"""Polygon rings simplified on the GPU (mrcnn_polygons_simplify; detection.simplify_polygons).  Every comparison is bit for bit against
the sequential host definition, which tests/test_polygons_simplify_host.py pins against a recursive restatement in Python integers:
out_ring_offsets, out_areas2, out_xy, out_src_index and the total, from host memory and from device tensors.

A ring of at most MRCNN_SIMPLIFY_LDS_VERTICES vertices is simplified by one workgroup in LDS, a larger one in that workgroup's carve of
a global scratch (kernels_simplify.hip): the rings below sit on both sides of that limit, in one call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import simplify_cases as SC
import tiles_cases as TC
import unite_cases as UC

pytestmark = pytest.mark.gpu
SHAPE = SC.SHAPE


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _both_memspaces_equal_the_definition(offs, xy, tol, what):
    """the device entry from host memory and from device tensors against the host entry -> the host's arrays"""
    D = _det()
    want = SC.simplify_host(offs, xy, tol)
    got = D.simplify_polygons({"ring_offsets": offs, "xy": xy}, tol)
    assert isinstance(got["xy"], np.ndarray) and got["n_vertices"] == want["n_vertices"], what
    SC.assert_same(got, want, f"{what}, tolerance {tol}, host memory:")
    dev = D.simplify_polygons({"ring_offsets": _cuda(offs), "xy": _cuda(xy)}, tol)
    assert all(dev[k].is_cuda for k in SC.KEYS) and dev["n_vertices"] == want["n_vertices"], what
    SC.assert_same({k: dev[k].cpu().numpy() for k in SC.KEYS}, want, f"{what}, tolerance {tol}, device memory:")
    return want


# ---- 1. every CPU ring in one ragged call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0, 1, 3])
def test_one_ragged_call_over_all_the_cpu_rings(pkg, tol):
    names, offs, xy, n_traced = SC.rings()
    assert len(names) > 2400 and "all_equal/6" in names and "extreme" in names
    want = _both_memspaces_equal_the_definition(offs, xy, tol, "all rings")
    if tol == 0:                                                 # the identity on the traced rings
        V = int(offs[n_traced])
        np.testing.assert_array_equal(want["xy"][:V], xy[:V])
    else:
        assert want["n_vertices"] < len(xy) // 2


# ---- 2. both sides of the LDS limit ------------------------------------------------------------------------------------------------
def _disks_beside(limit):
    """Two staircase disks whose outlines have the vertex counts closest to `limit` from below (at most `limit`) and from above, by the
    host tracer's own count; radii searched round 4.69 r = limit."""
    radii = np.arange(0.209 * limit, 0.216 * limit, 0.25)
    planes = [SC.disk(float(r), cx=int(0.216 * limit) + 3) for r in radii]
    tr = SC.trace_planes(planes)
    ro, rr = tr["ring_offsets"], tr["rle_rings"]
    assert (np.diff(rr) == 1).all()
    counts = np.diff(ro)
    below = int(np.argmax(np.where(counts <= limit, counts, -1)))
    above = int(np.argmin(np.where(counts > limit, counts, 1 << 30)))
    ring = lambda k: tr["xy"][int(ro[k]):int(ro[k + 1])]
    return ring(below), ring(above)


def _long_rings():
    """A traced comb of 600 teeth (2404 vertices: its ties peel one tooth off per level, so the rounds grow with the ring, not with its
    logarithm) and 20 000 integer vertices scattered round a circle of radius 15 000"""
    comb = np.zeros((3, 1201), np.uint8)
    comb[0, :] = 1
    comb[1:, ::2] = 1
    tr = SC.trace_planes([comb])
    assert tr["n_rings"] == 1
    rng = np.random.default_rng(31)
    a = np.arange(20000) * (2 * np.pi / 20000)
    rad = 15000 + rng.integers(-3, 4, 20000)
    circle = np.stack((np.rint(16000 + rad * np.cos(a)), np.rint(16000 + rad * np.sin(a))), 1).astype(np.int32)
    return tr["xy"], circle


@pytest.mark.parametrize("tol", [0.5, 2])
def test_both_sides_of_the_lds_limit_in_one_call(pkg, tol):
    limit = _lib().SIMPLIFY_LDS_VERTICES
    below, above = _disks_beside(limit)
    assert limit - 8 <= len(below) <= limit < len(above) <= limit + 8, (len(below), len(above))
    comb, circle = _long_rings()
    four = np.array([(2, 1), (9, 1), (9, 6), (2, 6)], np.int32)
    rings = [below, four, above, np.zeros((0, 2), np.int32), comb, below[::-1], circle, four]
    offs, xy = SC.flat_of(rings)
    sizes = np.diff(offs)
    assert list(sizes[[1, 3, 7]]) == [4, 0, 4] and sizes[4] == 2404 and sizes[6] == 20000
    assert (sizes > limit).sum() == 3 and ((sizes > 4) & (sizes <= limit)).sum() == 2               # both paths are taken
    want = _both_memspaces_equal_the_definition(offs, xy, tol, "LDS limit")
    out = np.diff(want["ring_offsets"])
    assert list(out[[1, 3, 7]]) == [4, 0, 4] and (out[[0, 2, 5, 6]] < sizes[[0, 2, 5, 6]]).all() and (out[[0, 2, 6]] > 8).all() and out[4] <= sizes[4], out


# ---- 3. the largest coordinates and the largest E ------------------------------------------------------------------------------------
def test_the_extreme_ring_up_to_the_largest_tolerance(pkg):
    offs, xy = SC.flat_of([SC.EXTREME, SC.EXTREME[::-1], [(32767, 32767), (0, 0), (32767, 0), (0, 32767)]])
    kept = []
    for tol in SC.EXTREME_TOLERANCES:
        want = _both_memspaces_equal_the_definition(offs, xy, tol, "extreme")
        kept.append(int(want["ring_offsets"][1]))
    assert kept[0] > kept[2] > kept[3] == kept[-1] == 2, kept                                        # the 128-bit comparison falls both ways


# ---- 4. rings traced on the device, simplified where they lie ----------------------------------------------------------------------------
def _trace_and_simplify_in_place(counts_g, offs_g, sizes, slots, tol):
    """mrcnn_rle_to_polygons and mrcnn_polygons_simplify with MRCNN_DEVICE on the tensors another entry wrote; no vertex crosses to the
    host between the two.  -> (the traced rings, the simplified arrays), tensors"""
    import torch
    lib = _lib()
    L = lib.lib()
    B = len(sizes)
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    n = B * slots
    rle_rings = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    nr, nv = C.c_int64(0), C.c_int64(0)
    head = (counts_g.data_ptr(), offs_g.data_ptr(), B, slots, hs.ctypes.data, ws.ctypes.data, lib.DEVICE, rle_rings.data_ptr(), C.byref(nr), C.byref(nv))
    st = L.mrcnn_rle_to_polygons(*head, None, None, 0, None, 0)
    assert st == SHAPE and nr.value > 0, L.mrcnn_last_error().decode()
    R, V = nr.value, nv.value
    ro, ra, xy = (torch.full((m,), -7, dtype=dt, device="cuda") for m, dt in ((R + 1, torch.int64), (R, torch.int64), (2 * V, torch.int32)))
    lib.check(L.mrcnn_rle_to_polygons(*head, ro.data_ptr(), ra.data_ptr(), R, xy.data_ptr(), V))
    out_ro, a2 = torch.full((R + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((R,), -7, dtype=torch.int64, device="cuda")
    total = C.c_int64(-7)
    simplify = lambda oxy, src, cap: L.mrcnn_polygons_simplify(ro.data_ptr(), xy.data_ptr(), R, C.c_double(tol), lib.DEVICE, out_ro.data_ptr(), a2.data_ptr(),
                                                               oxy, src, C.byref(total), cap)
    st = simplify(None, None, 0)                                  # the size query
    assert st == SHAPE and 0 < total.value <= V and (a2 == -7).all(), L.mrcnn_last_error().decode()
    n_out = total.value
    out_xy, src = torch.full((2 * n_out,), -7, dtype=torch.int32, device="cuda"), torch.full((n_out,), -7, dtype=torch.int64, device="cuda")
    lib.check(simplify(out_xy.data_ptr(), src.data_ptr(), n_out))
    torch.cuda.synchronize()
    assert total.value == n_out
    return (ro, xy.reshape(V, 2)), {"ring_offsets": out_ro, "areas2": a2, "xy": out_xy.reshape(n_out, 2), "src_index": src}


def _equals_the_definition_of_the_copy(traced, got, tol, what):
    ro, xy = (t.cpu().numpy() for t in traced)
    want = SC.simplify_host(ro, xy, tol)
    SC.assert_same({k: got[k].cpu().numpy() for k in SC.KEYS}, want, what)
    return ro, xy, want


def test_the_rings_of_masks_rle_source_are_simplified_where_they_lie(pkg):
    import torch
    from test_gpu_render import MODEL_H, MODEL_W, _synthetic
    lib = _lib()
    L = lib.lib()
    sizes, rows = [(64, 48), (37, 53)], 100
    det, masks = _synthetic(sizes, rows=rows, seed=77)
    hs, ws = np.array([64, 37], np.int32), np.array([48, 53], np.int32)
    det_g, masks_g = _cuda(det), _cuda(masks)
    det_src = torch.zeros((2, rows, 6), dtype=torch.float32, device="cuda")
    offs_g = torch.zeros((2 * rows + 1,), dtype=torch.int64, device="cuda")
    capacity = 2 * rows * 64 * 53
    counts_g = torch.zeros((capacity,), dtype=torch.int32, device="cuda")
    lib.check(L.mrcnn_masks_rle_source(det_g.data_ptr(), masks_g.data_ptr(), 2, rows, 28, hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W, C.c_float(0.5),
                                       lib.DEVICE, det_src.data_ptr(), counts_g.data_ptr(), capacity, offs_g.data_ptr(), None, None))
    traced, got = _trace_and_simplify_in_place(counts_g, offs_g, sizes, rows, 1.0)
    ro, xy, want = _equals_the_definition_of_the_copy(traced, got, 1.0, "masks_rle_source")
    assert len(ro) - 1 > 150 and want["n_vertices"] < len(xy) and (want["areas2"] < 0).any()          # noise masks: many rings, holes among them


def test_the_rings_of_unite_tiles_are_simplified_where_they_lie(pkg):
    D = _det()
    sc = next(s for s in UC.scenes() if s["name"] == "two_images")
    resident = []
    D._merge_tiles(False, _cuda(sc["det"]), _cuda(sc["masks"]), sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, sc["max_out"], unite=True,
                   resident=resident)
    counts_g, offs_g = resident[0]
    assert counts_g.is_cuda and offs_g.is_cuda
    sizes = [tuple(s) for s in sc["sizes"]]
    traced, got = _trace_and_simplify_in_place(counts_g, offs_g, sizes, sc["max_out"], 1.5)
    ro, xy, want = _equals_the_definition_of_the_copy(traced, got, 1.5, "unite_tiles")
    assert len(ro) - 1 >= 2 and 0 < want["n_vertices"] <= len(xy)
    # the binding on the same tensors: the pair is traced and simplified on the device, tensors come back
    flat = D.rle_to_polygons((counts_g, offs_g), sizes, flat=True, tolerance=1.5)
    assert flat["xy"].is_cuda and flat["areas2"].is_cuda and flat["n_vertices"] == want["n_vertices"]
    SC.assert_same({k: flat[k].cpu().numpy() for k in SC.KEYS}, want, "rle_to_polygons(tolerance)")
    plain = D.rle_to_polygons((counts_g, offs_g), sizes, flat=True)
    np.testing.assert_array_equal(flat["ring_areas"].cpu().numpy(), plain["ring_areas"].cpu().numpy())   # the original pixel areas


# ---- 5. the interface on the device ---------------------------------------------------------------------------------------------------
def _device_call(offs, xy, tol, cap, fill=-9):
    import torch
    lib = _lib()
    L = lib.lib()
    R = len(offs) - 1
    bufs = [torch.full((m,), fill, dtype=dt, device="cuda") for m, dt in ((R + 1, torch.int64), (max(1, R), torch.int64), (max(1, 2 * cap), torch.int32),
                                                                          (max(1, cap), torch.int64))]
    total = C.c_int64(fill)
    offs_g, xy_g = _cuda(offs), _cuda(xy)
    st = L.mrcnn_polygons_simplify(offs_g.data_ptr(), xy_g.data_ptr(), R, C.c_double(tol), lib.DEVICE, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                   bufs[3].data_ptr(), C.byref(total), cap)
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs], total.value


def _few_rings():
    hand = dict(SC.hand_made())
    return SC.flat_of([hand["collinear"], hand["m2"], hand["distance_tie"], hand["m0"], hand["rectangle"]])


def test_the_capacity_protocol_on_the_device(pkg):
    offs, xy = _few_rings()
    want = SC.simplify_host(offs, xy, 1.0)
    need = want["n_vertices"]
    assert 8 < need < len(xy)
    for cap in (need - 1, 1, 0):
        st, msg, (ro, a2, oxy, src), total = _device_call(offs, xy, 1.0, cap)
        assert st == SHAPE and f"vertex_capacity >= {need}" in msg, msg
        np.testing.assert_array_equal(ro, want["ring_offsets"])                                      # always written
        assert total == need and (a2 == -9).all() and (oxy == -9).all() and (src == -9).all()
    st, msg, (ro, a2, oxy, src), total = _device_call(offs, xy, 1.0, need + 5)                       # larger than needed: the rest stays
    assert st == 0 and total == need, msg
    np.testing.assert_array_equal(oxy[:2 * need].reshape(-1, 2), want["xy"])
    np.testing.assert_array_equal(src[:need], want["src_index"])
    np.testing.assert_array_equal(a2, want["areas2"])
    assert (oxy[2 * need:] == -9).all() and (src[need:] == -9).all()


def test_a_bad_ring_on_the_device_is_named_and_nothing_is_written(pkg):
    offs, xy = _few_rings()
    at = int(offs[2]) + 3                                        # a vertex of ring 2
    for value, col in ((-1, 0), (32768, 1)):
        bad = xy.copy()
        bad[at, col] = value
        st, msg, bufs, total = _device_call(offs, bad, 1.0, len(xy))
        assert st == SHAPE and "ring 2 " in msg and "0..32767" in msg, msg
        assert all((b == -9).all() for b in bufs) and total == -9
    worse = offs.copy()
    worse[4] = offs[3] - 2                                       # ring 3 ends before it starts
    st, msg, bufs, total = _device_call(worse, xy, 1.0, len(xy))
    assert st == SHAPE and "at ring 3" in msg, msg
    assert all((b == -9).all() for b in bufs) and total == -9


# ---- 6. the model's own rings ----------------------------------------------------------------------------------------------------------
def test_predict_tiled_hands_its_masks_on_as_simplified_rings(pkg, small_model):
    d, _cfg = small_model
    D = _det()
    m = importlib.import_module("mask-rcnn-coreml_amd.models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25)
    plain = m.predict_tiled(images, polygons=True, **kw)
    rings, areas = m.predict_tiled(images, polygons=True, tolerance=1.0, **kw)[4]
    w_rings, w_areas = D.simplify_polygons_host(plain[4], 1.0)
    before = after = 0
    for b in range(2):
        for i in range(6):
            assert len(rings[b][i]) == len(w_rings[b][i]) == len(plain[4][0][b][i])
            assert all(np.array_equal(a, c) for a, c in zip(rings[b][i], w_rings[b][i]))
            np.testing.assert_array_equal(areas[b][i], plain[4][1][b][i])                            # the pixel areas, not the simplified ones
            np.testing.assert_array_equal(areas[b][i], w_areas[b][i])
            before += sum(len(r) for r in plain[4][0][b][i])
            after += sum(len(r) for r in rings[b][i])
    assert 0 < after < before, (after, before)
    res = m.predict_tiled([_cuda(im) for im in images], polygons=True, tolerance=1.0, **kw)           # CUDA images: traced and simplified on the device
    assert all(np.array_equal(a, c) for b in range(2) for i in range(6) for a, c in zip(res[4][0][b][i], w_rings[b][i]))
    # coco_results: tracing and simplifying itself, simplifying the rings it is given, and taking simplified rings as they are
    sizes, ids, CR = [(200, 333), (300, 260)], [1, 2], _cr()
    given = CR.coco_results(ids, plain[0], plain[3], sizes, segmentation="polygon", polygons=(w_rings, w_areas))
    assert CR.coco_results(ids, plain[0], plain[3], sizes, segmentation="polygon", polygons=plain[4], tolerance=1.0) == given
    assert CR.coco_results(ids, plain[0], plain[3], sizes, segmentation="polygon", tolerance=1.0) == given
    assert any(r["segmentation"] for r in given)
