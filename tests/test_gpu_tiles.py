"""Tiled prediction on the GPU.  MaskRCNN.predict_tiles (mrcnn_maskrcnn_predict_tiles — windows of large images, each letterboxed with
its own geometry, the images staged once and the windows never cut out) against predict_images on contiguous crops; the device merge
(mrcnn_merge_tiles) against its host definition (mrcnn_merge_tiles_host, itself pinned against a brute-force restatement in
tests/test_tiles_host.py) on real records and on every scene of tests/tiles_cases.py; the same window listed twice; predict_tiled
end to end.  Every comparison is bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tiles_cases as TC
from conftest import rand_images

pytestmark = pytest.mark.gpu

SIZES = [(200, 333), (300, 260)]


def _models():
    return importlib.import_module("mask-rcnn-coreml_amd.models")


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _table():
    """8 windows of the model's size over image 0 (two of them shifted inward), 96x160 and 300x200 windows of image 1: 13 tiles of
    two images, interleaved — with max_batch = 4 that is three full predicts and a last one of a single tile."""
    a = _det().tile_plan(200, 333, (128, 128), (32, 32), image=0)
    b = np.array([[1, 0, 0, 96, 160], [1, 101, 57, 96, 160], [1, 204, 100, 96, 160], [1, 0, 0, 300, 200], [1, 0, 60, 300, 200]], np.int32)
    assert a.shape[0] == 8
    return np.concatenate([a[:3], b[:2], a[3:6], b[2:4], a[6:], b[4:]])


def _images():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


@pytest.fixture(scope="module", params=["f32x3", "f16"])
def records(request, pkg, small_model):
    import torch
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=4, compute_dtype=request.param)
    images, tiles = _images(), _table()
    plain = rand_images(2, cfg.image_height, cfg.image_width, seed=4)
    before = m.predict(plain)
    det, mask = m.predict_tiles(images, tiles)
    after = m.predict(plain)
    crops = [np.ascontiguousarray(images[i][y:y + h, x:x + w]) for i, y, x, h, w in tiles.tolist()]
    alone = [m.predict_images([c]) for c in crops]                       # the contract: window t ALONE
    dev = [torch.from_numpy(im).cuda() for im in images]
    det_g, mask_g = m.predict_tiles(dev, tiles)
    return dict(mode=request.param, m=m, images=images, tiles=tiles, det=det, mask=mask, before=before, after=after, alone=alone,
                det_g=det_g, mask_g=mask_g, dev=dev)


def test_predict_tiles_equals_predict_images_on_crops(records):
    r = records
    T = r["tiles"].shape[0]
    assert T == 13 and T > 4 and T % 4 != 0 and set(r["tiles"][:, 0].tolist()) == {0, 1}
    assert r["det"].shape == (T, r["m"].max_detections, 6) and r["mask"].shape[:2] == (T, r["m"].max_detections)
    assert (r["det"][..., 5] > 0).any(), "no detection at all: the comparison has no teeth"
    for t in range(T):
        np.testing.assert_array_equal(r["det"][t], r["alone"][t][0][0], err_msg=f"{r['mode']}: detections of tile {t} {r['tiles'][t]}")
        np.testing.assert_array_equal(r["mask"][t], r["alone"][t][1][0], err_msg=f"{r['mode']}: masks of tile {t} {r['tiles'][t]}")


def test_device_images_give_the_host_runs_bits_and_no_state_is_left(records):
    r = records
    assert r["det_g"].is_cuda and r["mask_g"].is_cuda
    np.testing.assert_array_equal(r["det_g"].cpu().numpy(), r["det"])
    np.testing.assert_array_equal(r["mask_g"].cpu().numpy(), r["mask"])
    for t, im in zip(r["dev"], r["images"]):                             # read in place, never written
        np.testing.assert_array_equal(t.cpu().numpy(), im)
    np.testing.assert_array_equal(r["after"][0], r["before"][0])
    np.testing.assert_array_equal(r["after"][1], r["before"][1])


def _same(got, want, tag):
    g_src, g_source, g_n, g_rles, g_areas, g_boxes = got
    w_src, w_source, w_n, w_rles, w_areas, w_boxes = want
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    np.testing.assert_array_equal(host(g_source), w_source, err_msg=str(tag))
    np.testing.assert_array_equal(host(g_n), w_n, err_msg=str(tag))
    np.testing.assert_array_equal(host(g_src).view(np.uint32), w_src.view(np.uint32), err_msg=str(tag))
    np.testing.assert_array_equal(host(g_areas).view(np.uint32), w_areas, err_msg=str(tag))
    np.testing.assert_array_equal(host(g_boxes), w_boxes, err_msg=str(tag))
    assert len(g_rles) == len(w_rles)
    for b, (gb, wb) in enumerate(zip(g_rles, w_rles)):
        assert len(gb) == len(wb)
        for j, (g, w) in enumerate(zip(gb, wb)):
            assert g["size"] == w["size"]
            np.testing.assert_array_equal(g["counts"], w["counts"], err_msg=str(tag + (b, j)))


CONFIGS = [("iou", 0.5, None), ("ios", 0.5, None), ("iou", 0.25, 3), ("ios", 0.75, 3)]


def test_merge_equals_the_host_definition_on_real_records(records):
    import torch
    D, r = _det(), records
    H = W = TC.MODEL
    for metric, thr, max_out in CONFIGS:
        want = D.merge_tiles_host(r["det"], r["mask"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out)
        _same(D.merge_tiles(r["det"], r["mask"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out), want, (r["mode"], metric, thr, max_out, "host"))
        got = D.merge_tiles(r["det_g"], r["mask_g"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out)
        assert all(torch.is_tensor(x) and x.is_cuda for x in (got[0], got[1], got[2], got[4], got[5]))
        _same(got, want, (r["mode"], metric, thr, max_out, "device"))
        eligible = int((want[1] >= 0).sum())
        assert eligible > 0


def test_merge_equals_the_host_definition_on_every_scene(pkg):
    D = _det()
    for sc in TC.scenes():
        cfgs = list(dict.fromkeys([(sc["metric"], sc["match_threshold"], sc["max_out"]), ("iou", 0.5, sc["max_out"]), ("ios", 0.5, sc["max_out"]),
                                   ("iou", 0.75, 2)] + [(m, t, sc["max_out"]) for (m, t) in sc["expect"]]))
        for metric, thr, max_out in cfgs:
            want = D.merge_tiles_host(sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, metric, thr, max_out)
            got = D.merge_tiles(sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, metric, thr, max_out)
            _same(got, want, (sc["name"], metric, thr, max_out))
            if (metric, thr) in sc["expect"]:
                for b, keep in enumerate(sc["expect"][(metric, thr)]):
                    assert got[1][b][got[1][b] >= 0].tolist() == keep[:max_out] and got[2][b] == len(keep)


def test_merge_size_query_then_exact_capacity(records):
    lib, r = _lib(), records
    L = lib.lib()
    T, rows = r["det"].shape[:2]
    hs, ws = np.array([s[0] for s in SIZES], np.int32), np.array([s[1] for s in SIZES], np.int32)
    max_out, B = 5, 2
    slots = B * max_out
    want = _det().merge_tiles_host(r["det"], r["mask"], r["tiles"], SIZES, TC.MODEL, TC.MODEL, 0.5, "ios", 0.5, max_out)
    src, source, nk = np.zeros((slots, 6), np.float32), np.zeros(slots, np.int32), np.zeros(B, np.int32)
    offs, areas, boxes = np.zeros(slots + 1, np.int64), np.zeros(slots, np.uint32), np.zeros((slots, 4), np.int32)
    tp = np.ascontiguousarray(r["tiles"]).ctypes.data_as(C.POINTER(lib.Tile))

    def call(counts, cap):
        return L.mrcnn_merge_tiles(r["det"].ctypes.data, r["mask"].ctypes.data, tp, T, rows, r["mask"].shape[2], hs.ctypes.data, ws.ctypes.data, B, TC.MODEL,
                                   TC.MODEL, C.c_float(0.5), lib.MATCH_IOS, 0.5, max_out, lib.HOST, src.ctypes.data, source.ctypes.data, nk.ctypes.data,
                                   counts, cap, offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data)
    assert call(None, 0) == 4                                            # the size query: MRCNN_ERR_SHAPE, everything but counts written
    need = int(offs[slots])
    assert f"capacity >= {need}" in L.mrcnn_last_error().decode()
    np.testing.assert_array_equal(source.reshape(B, max_out), want[1])
    np.testing.assert_array_equal(nk, want[2])
    counts = np.full(need + 4, 0xAAAAAAAA, np.uint32)
    assert call(counts.ctypes.data, need - 1) == 4 and (counts == 0xAAAAAAAA).all()
    assert call(counts.ctypes.data, need) == 0, L.mrcnn_last_error()
    assert (counts[need:] == 0xAAAAAAAA).all()
    flat = np.concatenate([w["counts"] for b in want[3] for w in b])
    np.testing.assert_array_equal(counts[:need], flat)
    np.testing.assert_array_equal(areas.reshape(B, max_out), want[4])
    np.testing.assert_array_equal(boxes.reshape(B, max_out, 4), want[5])


def test_the_same_window_twice(records):
    """Every candidate of the second copy that sets a pixel meets its twin — same class, another tile, the same plane — earlier in the
    order and is dropped by it; what is kept is the first copy, mapped as paste_masks_source maps the tile alone, shifted by the
    window's origin."""
    D, r = _det(), records
    CR = importlib.import_module("mask-rcnn-coreml_amd.coco_results")
    t = max(range(8), key=lambda i: int((r["det"][[0, 1, 2, 5, 6, 7, 10, 11][i]][:, 5] > 0).sum()))         # the fullest 128 x 128 window of image 0
    t = [0, 1, 2, 5, 6, 7, 10, 11][t]
    img, y0, x0, th, tw = r["tiles"][t].tolist()
    assert img == 0 and (th, tw) == (128, 128)
    h, w = SIZES[0]
    rows = r["det"].shape[1]
    det2, mask2 = np.stack([r["det"][t]] * 2), np.stack([r["mask"][t]] * 2)
    tiles2 = np.stack([r["tiles"][t]] * 2)
    tile_src, planes = D.paste_masks_source(det2[:1], mask2[:1], [(th, tw)], TC.MODEL, TC.MODEL, 0.5)
    tile_src, planes = tile_src[0], planes[0]
    box = lambda q: (int(np.around(np.float64(q[0]) * (th - 1))), int(np.around(np.float64(q[1]) * (tw - 1))),
                     int(np.around(np.float64(q[2]) * (th - 1) + 1.0)), int(np.around(np.float64(q[3]) * (tw - 1) + 1.0)))
    eligible = [i for i in range(rows) if tile_src[i, 5] > 0 and box(tile_src[i])[2] > box(tile_src[i])[0] and box(tile_src[i])[3] > box(tile_src[i])[1]]
    solid = [i for i in eligible if planes[i].any()]
    assert solid, "the window has no detection with a mask: the test has no teeth"
    src, source, n_kept, rles, areas, _ = D.merge_tiles(det2, mask2, tiles2, [SIZES[0]], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, 2 * rows)
    empty_twins = [rows + i for i in eligible if not planes[i].any()]                                       # m = 0/0 = 0: they stay
    want = sorted(eligible + empty_twins, key=lambda k: (-float(det2[0, k % rows, 5]), k))
    assert n_kept[0] == len(want) and source[0][:len(want)].tolist() == want and (source[0][len(want):] == -1).all()
    assert all(rows + i not in source[0].tolist() for i in solid)
    hy, wx = h - 1, w - 1
    for j, k in enumerate(want):
        i = k % rows
        by1, bx1, by2, bx2 = box(tile_src[i])
        row = np.array([np.float32((by1 + y0) / hy), np.float32((bx1 + x0) / wx), np.float32((by2 + y0 - 1) / hy), np.float32((bx2 + x0 - 1) / wx),
                        tile_src[i, 4], tile_src[i, 5]], np.float32)
        np.testing.assert_array_equal(src[0, j].view(np.uint32), row.view(np.uint32))
        full = np.zeros((h, w), np.uint8)
        full[y0:y0 + th, x0:x0 + tw] = planes[i]
        np.testing.assert_array_equal(CR.rle_decode(rles[0][j]), full)
        assert int(areas[0, j]) == int(full.sum())


def test_predict_tiled_is_its_three_steps(records):
    D, r = _det(), records
    m = r["m"]
    H, W = m.image_height, m.image_width
    tiles = np.concatenate([D.tile_plan(h, w, (H, W), (32, 48), b) for b, (h, w) in enumerate(SIZES)])
    det, mask = m.predict_tiles(r["images"], tiles)
    want = D.merge_tiles(det, mask, tiles, SIZES, H, W, 0.5, "ios", 0.5, 6)
    got = m.predict_tiled(r["images"], tile=None, overlap=(32, 48), metric="ios", match_threshold=0.5, max_out=6)
    assert len(got) == 4
    _same(got + want[4:], want, (r["mode"], "predict_tiled"))
    assert (got[1] >= 0).any()
