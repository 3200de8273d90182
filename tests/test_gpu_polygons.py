"""Run-length masks to polygon rings on the GPU (mrcnn_rle_to_polygons; detection.rle_to_polygons).  Every comparison is bit for bit
against the sequential host definition, which tests/test_polygons_host.py pins against a naive restatement: rle_rings, ring_offsets,
ring_areas, xy and the two totals, from host memory and from device tensors.

An RLE of at most MRCNN_POLYGON_LDS_CORNERS corners is traced by one workgroup in LDS, a larger one in global memory
(kernels_polygons.hip): the planes below sit on both sides of that limit, in one call, and one of them needs a much larger padded
slice than the other."""
import ctypes as C
import importlib

import numpy as np
import pytest

import polygons_cases as PC
import tiles_cases as TC
import unite_cases as UC

pytestmark = pytest.mark.gpu
SHAPE = PC.SHAPE


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _flat(rows):
    counts = np.concatenate([np.asarray(r["counts"], np.uint32) for row in rows for r in row])
    offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rows for r in row]))).astype(np.int64)
    return counts, offs


def _both_memspaces_equal_the_definition(rows, sizes, what):
    """rows[b][i] on images of `sizes`: the device entry from host memory and from device tensors against the host entry.  -> the host's arrays"""
    D = _det()
    want = D.rle_to_polygons_host(rows, sizes, flat=True)
    got = D.rle_to_polygons(rows, sizes, flat=True)
    assert (got["n_rings"], got["n_vertices"]) == (want["n_rings"], want["n_vertices"]), what
    PC.assert_same(got, want, f"{what}, host memory:")
    counts, offs = _flat(rows)
    dev = D.rle_to_polygons((_cuda(counts.view(np.int32)), _cuda(offs)), sizes, flat=True)
    assert all(dev[k].is_cuda for k in ("rle_rings", "ring_offsets", "ring_areas", "xy")), what
    assert (dev["n_rings"], dev["n_vertices"]) == (want["n_rings"], want["n_vertices"]), what
    PC.assert_same({k: dev[k].cpu().numpy() for k in ("rle_rings", "ring_offsets", "ring_areas", "xy")}, want, f"{what}, device memory:")
    return want


# ---- 1. every CPU case in one ragged call --------------------------------------------------------------------------------------------
def test_one_ragged_call_over_all_the_cpu_cases(pkg):
    """Images of mixed sizes with 8 slots each: the masks of one size six at a time, an empty mask in slots 1 and 4 and wherever a size
    runs out of masks."""
    by_size = {}
    for _name, rle in PC.cases():
        by_size.setdefault(tuple(rle["size"]), []).append(rle)
    rows, sizes = [], []
    for (h, w), rles in sorted(by_size.items()):
        empty = {"size": [h, w], "counts": np.array([h * w], np.uint32)}
        for at in range(0, len(rles), 6):
            six = rles[at:at + 6] + [empty] * 6
            rows.append([six[0], empty, six[1], six[2], empty, six[3], six[4], six[5]])
            sizes.append((h, w))
    assert len(set(sizes)) > 100 and len(rows) > 200
    want = _both_memspaces_equal_the_definition(rows, sizes, "all cases")
    per = np.diff(want["rle_rings"]).reshape(len(rows), 8)
    assert (per[:, [1, 4]] == 0).all() and (per[:, 0] > 0).sum() > 150 and want["n_rings"] > 1500


# ---- 2. both sides of the LDS limit ------------------------------------------------------------------------------------------------
def _prefix_planes(limit):
    """Two 40 x 40 planes, the first t and t' pixels (row-major) of one seeded random plane: the corner counts closest to `limit` from
    below (at most `limit`) and from above, by the host definition's own count."""
    D = _det()
    noise = np.random.default_rng(5).random((40, 40)) < 0.5
    flat = noise.reshape(-1)
    planes = []
    for t in range(40 * 25, 40 * 40 + 1):
        p = np.zeros(40 * 40, np.uint8)
        p[:t] = flat[:t]
        planes.append(p.reshape(40, 40))
    res = D.rle_to_polygons_host([[_cr().rle_encode(p) for p in planes]], flat=True)
    ro, rr = res["ring_offsets"], res["rle_rings"]
    corners = np.array([int(ro[rr[k + 1]] - ro[rr[k]]) for k in range(len(planes))])
    below = int(np.argmax(np.where(corners <= limit, corners, -1)))
    above = int(np.argmin(np.where(corners > limit, corners, 1 << 30)))
    return planes[below], planes[above], int(corners[below]), int(corners[above])


def test_both_sides_of_the_lds_limit_in_one_call(pkg):
    limit = _lib().POLYGON_LDS_CORNERS
    below, above, n_below, n_above = _prefix_planes(limit)
    assert limit - 8 <= n_below <= limit < n_above <= limit + 8, (n_below, n_above)
    enc = _cr().rle_encode
    small = np.zeros((40, 40), np.uint8)
    small[3:9, 4:30] = 1
    board = np.indices((96, 96)).sum(0) % 2                                 # 4608 single pixels: 18432 corners, a slice of 32768
    rows = [[enc(below), enc(above), enc(small), enc(np.zeros((40, 40)))], [enc(board), enc(1 - board), enc(np.ones((96, 96))), enc(board.T[::-1] | board)]]
    sizes = [(40, 40), (96, 96)]
    want = _both_memspaces_equal_the_definition(rows, sizes, "LDS limit")
    ro, rr = want["ring_offsets"], want["rle_rings"]
    corners = [int(ro[rr[k + 1]] - ro[rr[k]]) for k in range(8)]
    assert corners[:4] == [n_below, n_above, 4, 0] and corners[4] == 18432 and corners[6] == 4, corners       # both paths were taken
    assert sum(c > limit for c in corners) >= 3 and sum(0 < c <= limit for c in corners) >= 3


# ---- 3. extreme planes -----------------------------------------------------------------------------------------------------------------
def test_the_longest_and_the_widest_plane(pkg):
    tall = {"size": [32767, 2], "counts": np.array([0, 5, 32000, 762 + 32767 - 10, 9, 1], np.uint32)}      # from pixel 0, across the column end, the last pixel
    wide = {"size": [2, 32767], "counts": np.array([1, 3, 65000, 1, 2 * 32767 - 65005 - 2, 2], np.uint32)}  # up to the last pixel
    full_t = {"size": [32767, 2], "counts": np.array([0, 65534], np.uint32)}
    full_w = {"size": [2, 32767], "counts": np.array([0, 65534], np.uint32)}
    for r in (tall, wide):
        assert int(r["counts"].sum()) == 65534
    want = _both_memspaces_equal_the_definition([[tall, full_t], [wide, full_w]], [(32767, 2), (2, 32767)], "extreme planes")
    assert int(want["xy"][:, 0].max()) == 32767 and int(want["xy"][:, 1].max()) == 32767
    assert list(want["ring_areas"][[int(want["rle_rings"][1]), int(want["rle_rings"][3])]]) == [65534, 65534]


# ---- 4. a realistic batch, traced where it lies ---------------------------------------------------------------------------------------
def _trace_in_place(counts_g, offs_g, sizes, slots):
    """mrcnn_rle_to_polygons with MRCNN_DEVICE on the tensors another entry wrote: the size query, then the call -> numpy arrays"""
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
    torch.cuda.synchronize()
    assert (nr.value, nv.value) == (R, V)
    return {"rle_rings": rle_rings.cpu().numpy(), "ring_offsets": ro.cpu().numpy(), "ring_areas": ra.cpu().numpy(), "xy": xy.cpu().numpy().reshape(V, 2)}


def test_the_runs_masks_rle_source_wrote_are_traced_in_place(pkg):
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
    got = _trace_in_place(counts_g, offs_g, sizes, rows)
    offs = offs_g.cpu().numpy()
    counts = counts_g.cpu().numpy().view(np.uint32)[:offs[-1]]
    rles = [[{"size": list(sizes[b]), "counts": counts[offs[b * rows + i]:offs[b * rows + i + 1]]} for i in range(rows)] for b in range(2)]
    want = _det().rle_to_polygons_host(rles, sizes, flat=True)
    PC.assert_same(got, want, "masks_rle_source")
    assert want["n_rings"] > 150 and (want["ring_areas"] < 0).any()                                  # noise masks: many rings, holes among them


def test_the_runs_unite_tiles_wrote_are_traced_in_place(pkg):
    D = _det()
    sc = next(s for s in UC.scenes() if s["name"] == "two_images")
    resident = []
    out = D._merge_tiles(False, _cuda(sc["det"]), _cuda(sc["masks"]), sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, sc["max_out"], unite=True,
                         resident=resident)
    counts_g, offs_g = resident[0]
    assert counts_g.is_cuda and offs_g.is_cuda
    sizes = [tuple(s) for s in sc["sizes"]]
    got = _trace_in_place(counts_g, offs_g, sizes, sc["max_out"])
    want = D.rle_to_polygons_host(out[3], sizes, flat=True)
    PC.assert_same(got, want, "unite_tiles")
    assert want["n_rings"] >= 2 and int(want["ring_areas"].sum()) == int(out[4].cpu().numpy().view(np.uint32).sum())


# ---- 5. the interface on the device ---------------------------------------------------------------------------------------------------
def _device_call(counts, offs, sizes, slots, rc, vc, fill=-9):
    import torch
    lib = _lib()
    L = lib.lib()
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    n = len(sizes) * slots
    bufs = [torch.full((m,), fill, dtype=dt, device="cuda") for m, dt in ((n + 1, torch.int64), (rc + 1, torch.int64), (max(1, rc), torch.int64),
                                                                          (max(1, 2 * vc), torch.int32))]
    nr, nv = C.c_int64(fill), C.c_int64(fill)
    counts_g, offs_g = _cuda(counts.view(np.int32)), _cuda(offs)
    st = L.mrcnn_rle_to_polygons(counts_g.data_ptr(), offs_g.data_ptr(), len(sizes), slots, hs.ctypes.data, ws.ctypes.data, lib.DEVICE,
                                 bufs[0].data_ptr(), C.byref(nr), C.byref(nv), bufs[1].data_ptr(), bufs[2].data_ptr(), rc, bufs[3].data_ptr(), vc)
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs], nr.value, nv.value


def test_the_capacity_protocol_on_the_device(pkg):
    cases = dict(PC.cases())
    rles = [cases["hole_with_island"], {"size": [9, 11], "counts": np.array([99], np.uint32)}]
    counts, offs = _flat([rles])
    for rc, vc in ((3, 16), (4, 15), (0, 0)):
        st, msg, (rle_rings, ro, ra, xy), nr, nv = _device_call(counts, offs, [(9, 11)], 2, rc, vc)
        assert st == SHAPE and "ring_capacity >= 4" in msg and "vertex_capacity >= 16" in msg, msg
        assert list(rle_rings) == [0, 4, 4] and (nr, nv) == (4, 16)
        assert (ro == -9).all() and (ra == -9).all() and (xy == -9).all()
    st, msg, (rle_rings, ro, ra, xy), nr, nv = _device_call(counts, offs, [(9, 11)], 2, 6, 20)
    assert st == 0, msg
    assert list(ro[:5]) == [0, 4, 8, 12, 16] and (ro[5:] == -9).all() and list(ra[:4]) == [63, -35, 9, -1] and (ra[4:] == -9).all() and (xy[32:] == -9).all()


def test_a_bad_rle_on_the_device_is_named_and_nothing_is_written(pkg):
    cases = dict(PC.cases())
    rles = [cases["checkerboard"], cases["checkerboard/other"], cases["checkerboard"]]
    counts, offs = _flat([rles])
    for delta in (1, -1):
        bad = counts.copy()
        bad[offs[1] + 3] = np.uint32(int(bad[offs[1] + 3]) + delta)
        st, msg, bufs, nr, nv = _device_call(bad, offs, [(8, 9)], 3, 64, 512)
        assert st == SHAPE and "RLE 1 (image 0, slot 1)" in msg and f"sums to {72 + delta} pixels" in msg, msg
        assert all((b == -9).all() for b in bufs) and (nr, nv) == (-9, -9)


def test_predict_tiled_hands_its_masks_on_as_rings(pkg, small_model):
    d, _cfg = small_model
    m = importlib.import_module("mask-rcnn-coreml_amd.models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25)
    det_src, source, _n, rles, (rings, areas) = m.predict_tiled(images, polygons=True, **kw)
    assert (source >= 0).any()
    w_rings, w_areas = _det().rle_to_polygons_host(rles)
    for b in range(2):
        for i in range(6):
            assert len(rings[b][i]) == len(w_rings[b][i]) and all(np.array_equal(a, c) for a, c in zip(rings[b][i], w_rings[b][i]))
            np.testing.assert_array_equal(areas[b][i], w_areas[b][i])
            assert int(areas[b][i].sum()) == int(_cr().rle_decode(rles[b][i]).sum())
    res = m.predict_tiled([_cuda(im) for im in images], polygons=True, **kw)                         # CUDA images: the runs are traced on the device
    assert all(np.array_equal(a, c) for b in range(2) for i in range(6) for a, c in zip(res[4][0][b][i], w_rings[b][i]))
