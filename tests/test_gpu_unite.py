"""Uniting the cut parts of objects across tiles on the GPU: mrcnn_unite_tiles against its host definition (mrcnn_unite_tiles_host,
itself pinned against a brute-force restatement in tests/test_unite_host.py) on every scene of tests/unite_cases.py and on real records
of the small model, from numpy arrays and from device tensors; the capacity protocol; predict_tiled with and without the flag.  Every
comparison is bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tiles_cases as TC
import unite_cases as UC

pytestmark = pytest.mark.gpu

SIZES = [(200, 333), (300, 260)]


def _models():
    return importlib.import_module("mask-rcnn-coreml_amd.models")


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _table():
    """8 windows of the model's size over image 0 (two of them shifted inward), 96x160 and 300x200 windows of image 1, interleaved."""
    a = _det().tile_plan(200, 333, (128, 128), (32, 32), image=0)
    b = np.array([[1, 0, 0, 96, 160], [1, 101, 57, 96, 160], [1, 204, 100, 96, 160], [1, 0, 0, 300, 200], [1, 0, 60, 300, 200]], np.int32)
    return np.concatenate([a[:3], b[:2], a[3:6], b[2:4], a[6:], b[4:]])


@pytest.fixture(scope="module", params=["f32x3", "f16"])
def records(request, pkg, small_model):
    import torch
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=4, compute_dtype=request.param)
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    tiles = _table()
    det, mask = m.predict_tiles(images, tiles)
    return dict(mode=request.param, m=m, images=images, tiles=tiles, det=det, mask=mask, det_g=torch.from_numpy(det).cuda(),
                mask_g=torch.from_numpy(mask).cuda())


def _same(got, want, tag):
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    names = ("det_src", "source", "n_kept", "rles", "areas", "bboxes", "n_parts", "group")
    assert len(got) == len(want) == 8
    for name, g, w in zip(names, got, want):
        if name == "rles":
            assert len(g) == len(w)
            for b, (gb, wb) in enumerate(zip(g, w)):
                assert len(gb) == len(wb)
                for j, (x, y) in enumerate(zip(gb, wb)):
                    assert x["size"] == y["size"]
                    np.testing.assert_array_equal(x["counts"], y["counts"], err_msg=str(tag + (b, j)))
        else:
            g = host(g)
            assert g.shape == w.shape, (name, tag)
            np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=str(tag + (name,)))


def test_unite_equals_the_host_definition_on_every_scene(pkg):
    D = _det()
    united = False
    for sc in UC.scenes():
        for metric, thr, max_out in UC.configs(sc):
            args = (sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, metric, thr, max_out)
            want = D.unite_tiles_host(*args)
            _same(D.unite_tiles(*args), want, (sc["name"], metric, thr, max_out))
            united |= bool((want[6] > 1).any())
    assert united


def test_the_hand_derived_numbers_on_the_device(pkg):
    D = _det()
    by_name = {sc["name"]: sc for sc in UC.scenes()}
    run = lambda name, metric, thr: D.unite_tiles(*(by_name[name][k] for k in ("det", "masks", "tiles", "sizes")), TC.MODEL, TC.MODEL, 0.5, metric, thr, 4)
    cut = run("cut_in_two", "iou", 0.5)
    assert cut[2][0] == 1 and int(cut[4][0, 0]) == 4000 and cut[5][0, 0].tolist() == [60, 30, 100, 40] and cut[6][0].tolist() == [2, 0, 0, 0]
    assert [int(a) for a in run("exactly_the_threshold", "iou", 0.5)[4][0, :2]] == [4000, 0]
    assert [int(a) for a in run("exactly_the_threshold", "iou", 0.75)[4][0, :2]] == [2720, 1920]
    assert run("full_height", "iou", 0.5)[3][0][0]["counts"].tolist() == [7680, 12800, 8192]
    chain = run("chain", "iou", 0.5)
    assert chain[1][0, 0] == UC.k(1, 0) and int(chain[4][0, 0]) == 10000 and chain[5][0, 0].tolist() == [20, 30, 250, 40]
    assert chain[7].reshape(-1)[[UC.k(1, 0), UC.k(2, 0), UC.k(0, 0)]].tolist() == [0, 0, 0] and chain[6][0, 0] == 3


CONFIGS = [("iou", 0.5, None), ("ios", 0.5, None), ("iou", 0.1, 3), ("ios", 0.25, 5)]


def test_unite_equals_the_host_definition_on_real_records(records):
    import torch
    D, r = _det(), records
    H = W = TC.MODEL
    for metric, thr, max_out in CONFIGS:
        want = D.unite_tiles_host(r["det"], r["mask"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out)
        assert (want[1] >= 0).any(), "no candidate at all: the comparison has no teeth"
        _same(D.unite_tiles(r["det"], r["mask"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out), want, (r["mode"], metric, thr, max_out, "host"))
        got = D.unite_tiles(r["det_g"], r["mask_g"], r["tiles"], SIZES, H, W, 0.5, metric, thr, max_out)
        assert all(torch.is_tensor(x) and x.is_cuda for x in got[:3] + got[4:])
        _same(got, want, (r["mode"], metric, thr, max_out, "device"))


def test_unite_size_query_then_exact_capacity_then_one_short(records):
    lib, r = _lib(), records
    L = lib.lib()
    T, rows = r["det"].shape[:2]
    hs, ws = np.array([s[0] for s in SIZES], np.int32), np.array([s[1] for s in SIZES], np.int32)
    max_out, B = 5, 2
    slots = B * max_out
    want = _det().unite_tiles_host(r["det"], r["mask"], r["tiles"], SIZES, TC.MODEL, TC.MODEL, 0.5, "ios", 0.25, max_out)
    src, source, nk = np.zeros((slots, 6), np.float32), np.zeros(slots, np.int32), np.zeros(B, np.int32)
    offs, areas, boxes = np.zeros(slots + 1, np.int64), np.zeros(slots, np.uint32), np.zeros((slots, 4), np.int32)
    parts, group = np.zeros(slots, np.int32), np.zeros(T * rows, np.int32)
    tp = np.ascontiguousarray(r["tiles"]).ctypes.data_as(C.POINTER(lib.Tile))

    def call(counts, cap, parts_p=parts.ctypes.data, group_p=group.ctypes.data):
        return L.mrcnn_unite_tiles(r["det"].ctypes.data, r["mask"].ctypes.data, tp, T, rows, r["mask"].shape[2], hs.ctypes.data, ws.ctypes.data, B, TC.MODEL,
                                   TC.MODEL, C.c_float(0.5), lib.MATCH_IOS, 0.25, max_out, lib.HOST, src.ctypes.data, source.ctypes.data, nk.ctypes.data,
                                   parts_p, group_p, counts, cap, offs.ctypes.data, areas.ctypes.data, boxes.ctypes.data)
    assert call(None, 0) == 4                                            # the size query: MRCNN_ERR_SHAPE, everything but counts written
    need = int(offs[slots])
    assert f"capacity >= {need}" in L.mrcnn_last_error().decode()
    np.testing.assert_array_equal(source.reshape(B, max_out), want[1])
    np.testing.assert_array_equal(nk, want[2])
    np.testing.assert_array_equal(parts.reshape(B, max_out), want[6])
    np.testing.assert_array_equal(group.reshape(T, rows), want[7])
    counts = np.full(need + 4, 0xAAAAAAAA, np.uint32)
    assert call(counts.ctypes.data, need) == 0, L.mrcnn_last_error()
    assert (counts[need:] == 0xAAAAAAAA).all()
    flat = np.concatenate([w["counts"] for b in want[3] for w in b])
    np.testing.assert_array_equal(counts[:need], flat)
    np.testing.assert_array_equal(areas.reshape(B, max_out), want[4])
    np.testing.assert_array_equal(boxes.reshape(B, max_out, 4), want[5])
    counts[:] = 0xAAAAAAAA
    assert call(counts.ctypes.data, need - 1, None, None) == 4 and (counts == 0xAAAAAAAA).all()           # one run short; n_parts and group may be NULL
    assert f"capacity >= {need}" in L.mrcnn_last_error().decode()


def test_predict_tiled_with_unite_is_its_three_steps(records):
    D, r = _det(), records
    m = r["m"]
    H, W = m.image_height, m.image_width
    tiles = np.concatenate([D.tile_plan(h, w, (H, W), (32, 48), b) for b, (h, w) in enumerate(SIZES)])
    det, mask = m.predict_tiles(r["images"], tiles)
    want = D.unite_tiles(det, mask, tiles, SIZES, H, W, 0.5, "iou", 0.25, 6)
    got = m.predict_tiled(r["images"], tile=None, overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25)
    assert len(got) == 4
    _same(got + want[4:], want, (r["mode"], "predict_tiled(unite=True)"))
    assert (got[1] >= 0).any()
    # without the flag: the merge, as before
    merged = D.merge_tiles(det, mask, tiles, SIZES, H, W, 0.5, "ios", 0.5, 6)
    plain = m.predict_tiled(r["images"], tile=None, overlap=(32, 48), metric="ios", match_threshold=0.5, max_out=6)
    assert len(plain) == 4
    for g, w in zip(plain[:3], merged[:3]):
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32))
    for gb, wb in zip(plain[3], merged[3]):
        for x, y in zip(gb, wb):
            np.testing.assert_array_equal(x["counts"], y["counts"])
