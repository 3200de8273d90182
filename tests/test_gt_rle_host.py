"""mrcnn_rle_from_polygons_batch without a GPU: the entry is declared, bound and exported; every argument error is answered before
the device is touched (so the codes below do not depend on whether a device is present); the Python layer of the resident ground
truth imports, and what exists without it is unchanged."""
import ctypes as C
import importlib
import inspect
import os

import numpy as np

from test_coco_eval_host import SMALL_SIZES, synthetic_dataset

INVALID, SHAPE = 1, 4


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def test_codes_are_the_headers():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maskrcnn_hip.h")).read()
    assert "MRCNN_ERR_INVALID = %d," % INVALID in header and "MRCNN_ERR_SHAPE = %d," % SHAPE in header


def test_symbol_declared_bound_and_exported():
    lib_mod = _mod("_lib")
    L = lib_mod.lib()
    assert "mrcnn_rle_from_polygons_batch" in lib_mod.EXPORTED_SYMBOLS and hasattr(L, "mrcnn_rle_from_polygons_batch")
    assert len(L.mrcnn_rle_from_polygons_batch.argtypes) == 12
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maskrcnn_hip.h")).read()
    assert "mrcnn_rle_from_polygons_batch(" in header and "MRCNN_POLY_LDS_TOGGLES 4096" in header
    assert _mod("coco_eval").LDS_TOGGLES == 4096


def _tables():
    xy = np.array([0, 0, 10, 0, 10, 10, 0, 10, 2, 2, 8, 2, 5, 9], np.float64)
    po = np.array([0, 4, 7], np.int64)
    ao = np.array([0, 1, 2], np.int64)
    hs = np.array([20, 30], np.int32)
    ws = np.array([25, 35], np.int32)
    return xy, po, ao, hs, ws


def _call(xy, po, ao, hs, ws, n=2, counts=None, capacity=0, ro="own"):
    L = _mod("_lib").lib()
    p = lambda a: None if a is None else a.ctypes.data
    own = np.zeros(n + 1, np.int64)
    st = L.mrcnn_rle_from_polygons_batch(p(xy), p(po), p(ao), n, p(hs), p(ws), 0, p(counts), capacity, p(own) if ro == "own" else None, None, None)
    return st, L.mrcnn_last_error().decode()


def test_argument_errors_come_before_the_device():
    xy, po, ao, hs, ws = _tables()
    # null tables
    assert _call(xy, po, None, hs, ws)[0] == INVALID
    assert _call(xy, None, ao, hs, ws)[0] == INVALID
    assert _call(None, po, ao, hs, ws)[0] == INVALID
    assert _call(xy, po, ao, None, ws)[0] == INVALID
    assert _call(xy, po, ao, hs, None)[0] == INVALID
    assert _call(xy, po, ao, hs, ws, ro=None)[0] == INVALID
    assert _call(xy, po, ao, hs, ws, counts=None, capacity=5)[0] == INVALID
    assert _call(xy, po, ao, hs, ws, n=-1)[0] == INVALID
    # decreasing offsets: the message names the annotation (and the polygon)
    st, msg = _call(xy, po, np.array([0, 2, 1], np.int64), hs, ws)
    assert st == INVALID and "annotation 1" in msg
    st, msg = _call(xy, np.array([0, 4, 3], np.int64), ao, hs, ws)
    assert st == INVALID and "polygon 0 of annotation 1" in msg
    assert _call(xy, po, np.array([-1, 1, 2], np.int64), hs, ws)[0] == INVALID
    # sides
    for bad in (0, 32768, -3):
        st, msg = _call(xy, po, ao, np.array([20, bad], np.int32), ws)
        assert st == SHAPE and "annotation 1" in msg and "1..32767" in msg
        st, msg = _call(xy, po, ao, hs, np.array([bad, 35], np.int32))
        assert st == SHAPE and "annotation 0" in msg
    # coordinates
    for bad in (np.nan, np.inf, -np.inf, 1e6, -2e7):
        x = xy.copy(); x[11] = bad
        st, msg = _call(x, po, ao, hs, ws)
        assert st == INVALID and "coordinate 3 of polygon 0 of annotation 1" in msg, (bad, st, msg)


def test_python_layer_without_a_gpu():
    CE, E = _mod("coco_eval"), _mod("evaluate")
    assert callable(CE.COCOGroundTruth.to_device) and callable(CE.rle_from_polygons_batch) and inspect.isclass(CE.DeviceGroundTruth)
    for fn in (CE.score, CE.score_batch):
        assert inspect.signature(fn).parameters["device_gt"].default is None
    assert inspect.signature(E.evaluate_coco_scored).parameters["device_gt"].default is False
    # a polygon of odd length is refused like rle_from_polygons refuses it, before any call into the library
    try:
        CE.rle_from_polygons_batch([[[0, 0, 4, 0, 4]]], [(8, 8)])
        raise AssertionError("accepted")
    except ValueError:
        pass
    # what the ground truth gives without to_device is what it gave: counts per annotation from the host entry, area from the file,
    # else from those counts
    ds, _ = synthetic_dataset(SMALL_SIZES[:3], seed=3)
    gt = CE.COCOGroundTruth(ds)
    for a in gt.annotations:
        c = gt.counts(a)
        h, w = gt.images[a["image_id"]]
        assert int(c.astype(np.int64).sum()) == h * w
        np.testing.assert_array_equal(c, CE.segmentation_to_counts(a["segmentation"], h, w))
        assert gt.area(a) == float(a["area"])
        b = dict(a, area=None)
        assert gt.area(b) == float(c[1::2].astype(np.int64).sum())
