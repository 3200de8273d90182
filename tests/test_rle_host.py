"""COCO run-length encoding, the parts that need no GPU: the compressed-string codec of the C library (mrcnn_rle_to_string /
mrcnn_rle_from_string) against a known answer and round trips, the numpy helpers rle_encode / rle_decode, the COCO results records,
and the new entries' presence in the header, the binding and the built library.  Every comparison is exact."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mrcnn_masks_rle_source", "mrcnn_rle_to_string", "mrcnn_rle_from_string")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def test_known_answer_both_directions(pkg):
    """Decoded by hand from the codec's rules: 40 takes two characters (X1), 4 goes out as 4 - 1 = 3, 5 as 5 - 40 = -35 (mN),
    21 as 21 - 5 = 16, whose bit 0x10 needs a second character (`0)."""
    CR = _cr()
    counts = np.array([6, 1, 40, 4, 5, 4, 5, 4, 21], np.uint32)
    text = "61X13mN000`0"
    assert int(counts.sum()) == 9 * 10 and len(text) == 12
    assert CR.rle_to_string(counts) == text
    got = CR.rle_from_string(text)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, counts)
    plane = CR.rle_decode({"size": [9, 10], "counts": text})             # a compressed RLE decodes too
    assert plane.shape == (9, 10) and int(plane.sum()) == 1 + 4 + 4 + 4
    np.testing.assert_array_equal(CR.rle_encode(plane)["counts"], counts)


def test_string_round_trips(pkg):
    CR = _cr()
    rng = np.random.default_rng(17)
    cases = [np.array([640 * 480], np.uint32), np.array([0, 640 * 480], np.uint32), np.array([0], np.uint32), np.zeros(0, np.uint32),
             np.array([0, 1, 1 << 20, (1 << 20) + 1, 3, (1 << 30) - 7, 1, 32767 * 32767, 2], np.uint32),
             np.array([0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 1], np.uint32)]
    for n in (1, 2, 3, 4, 5, 64, 1000):
        c = rng.integers(1, 1 << int(rng.integers(1, 31)), n).astype(np.uint32)
        if n % 2 == 0:
            c[0] = 0                                                     # pixel (0,0) set
        cases.append(c)
        big = rng.integers(1 << 20, 1 << 30, n).astype(np.uint32)        # counts above 2^20
        cases.append(big)
    for c in cases:
        s = CR.rle_to_string(c)
        assert all(48 <= ord(ch) < 112 for ch in s)
        np.testing.assert_array_equal(CR.rle_from_string(s), c)
        assert CR.rle_to_string(CR.rle_from_string(s)) == s


def test_string_entries_measure_and_refuse(pkg):
    lib = _lib()
    L = lib.lib()
    counts = np.array([6, 1, 40, 4, 5, 4, 5, 4, 21], np.uint32)
    n = C.c_int64(-1)
    assert L.mrcnn_rle_to_string(counts.ctypes.data, counts.size, None, 0, C.byref(n)) == 0 and n.value == 12       # measuring form
    buf = C.create_string_buffer(b"\x7f" * 16, 16)
    assert L.mrcnn_rle_to_string(counts.ctypes.data, counts.size, buf, 11, C.byref(n)) == 4 and n.value == 12       # one short: MRCNN_ERR_SHAPE
    assert buf.raw[11:] == b"\x7f" * 5                                                                              # nothing behind the capacity
    assert L.mrcnn_rle_to_string(counts.ctypes.data, counts.size, buf, 12, C.byref(n)) == 0 and buf.raw[:12] == b"61X13mN000`0"
    out = np.full(12, 0xAAAAAAAA, np.uint32)
    text = b"61X13mN000`0"
    assert L.mrcnn_rle_from_string(text, 12, None, 0, C.byref(n)) == 0 and n.value == 9
    assert L.mrcnn_rle_from_string(text, 12, out.ctypes.data, 8, C.byref(n)) == 4 and n.value == 9
    assert (out[8:] == 0xAAAAAAAA).all()
    assert L.mrcnn_rle_from_string(text, 12, out.ctypes.data, 9, C.byref(n)) == 0
    np.testing.assert_array_equal(out[:9], counts)
    assert L.mrcnn_rle_from_string(b"61X", 3, out.ctypes.data, 9, C.byref(n)) == 1                  # ends inside a value
    assert L.mrcnn_rle_from_string(b"6 1", 3, out.ctypes.data, 9, C.byref(n)) == 1                  # not a character of the code
    assert L.mrcnn_rle_from_string(b"N", 1, out.ctypes.data, 9, C.byref(n)) == 1                    # a negative count
    assert L.mrcnn_rle_to_string(counts.ctypes.data, counts.size, buf, 12, None) == 1


def test_encode_decode_planes(pkg):
    CR = _cr()
    # 3 x 4, written out: columns are (0,1,1) (1,1,0) (0,0,0) (0,1,0) → column-major 0 11 11 0 000 0 1 0 → runs 1, 4, 5, 1, 1
    plane = np.array([[0, 1, 0, 0],
                      [1, 1, 0, 1],
                      [1, 0, 0, 0]], np.uint8)
    rle = CR.rle_encode(plane)
    assert rle["size"] == [3, 4] and rle["counts"].dtype == np.uint32
    np.testing.assert_array_equal(rle["counts"], [1, 4, 5, 1, 1])
    np.testing.assert_array_equal(CR.rle_decode(rle), plane)
    first = plane.copy(); first[0, 0] = 1                                  # pixel (0,0) set: a leading zero-length run
    np.testing.assert_array_equal(CR.rle_encode(first)["counts"], [0, 5, 5, 1, 1])
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (2, 5), (37, 53), (1, 9), (9, 1)):
        for p in (np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8),
                  (rng.random((h, w)) < 0.05).astype(np.uint8)):
            rle = CR.rle_encode(p)
            c = rle["counts"]
            assert int(c.astype(np.int64).sum()) == h * w and (c[1:] > 0).all()
            got = CR.rle_decode(rle)
            assert got.dtype == np.uint8 and got.shape == (h, w)
            np.testing.assert_array_equal(got, p)
            np.testing.assert_array_equal(CR.rle_decode({"size": [h, w], "counts": CR.rle_to_string(c)}), p)
        np.testing.assert_array_equal(CR.rle_encode(np.zeros((h, w), np.uint8))["counts"], [h * w])
        np.testing.assert_array_equal(CR.rle_encode(np.ones((h, w), np.uint8))["counts"], [0, h * w])
    with pytest.raises(ValueError):
        CR.rle_decode({"size": [3, 4], "counts": np.array([5, 5], np.uint32)})


def test_coco_results_records(pkg):
    CR = _cr()
    sizes = [(11, 21), (8, 5)]
    det = np.zeros((2, 3, 6), np.float32)
    det[0, 0] = [0.2, 0.1, 0.5, 0.75, 3, 0.9]
    det[0, 1] = [0.0, 0.0, 1.0, 1.0, 7, 0.25]
    det[1, 0] = [3 / 7, 0.5, 3 / 7, 0.5, 2, 0.6]                           # a one-pixel box
    det[1, 2] = [0.1, 0.1, 0.9, 0.9, 4, 0.0]                               # score 0: never a record
    planes = [np.zeros((3, 11, 21), np.uint8), np.zeros((3, 8, 5), np.uint8)]
    planes[0][0, 2:6, 2:16] = 1
    planes[0][1, :, :] = 1
    planes[1][0, 3, 2] = 1
    rles = [[CR.rle_encode(p) for p in planes[b]] for b in range(2)]
    recs = CR.coco_results([42, np.int64(7)], det, rles, sizes)
    assert [r["image_id"] for r in recs] == [42, 42, 7] and all(type(r["image_id"]) is int for r in recs)
    for r in recs:
        assert sorted(r) == ["bbox", "category_id", "image_id", "score", "segmentation"]
        assert sorted(r["segmentation"]) == ["counts", "size"] and isinstance(r["segmentation"]["counts"], str)
    # bbox: denorm_boxes of the row at the image's size — around(y*(h-1)), around(x*(w-1)), far edge + 1 — as x, y, width, height
    assert recs[0]["bbox"] == [2.0, 2.0, 14.0, 4.0]                        # y 0.2*10 = 2 .. 0.5*10 + 1 = 6; x 0.1*20 = 2 .. 0.75*20 + 1 = 16
    assert recs[1]["bbox"] == [0.0, 0.0, 21.0, 11.0]
    assert recs[2]["bbox"] == [2.0, 3.0, 1.0, 1.0]                         # y 3/7*7 = 3 .. 4, x 0.5*4 = 2 .. 3
    assert [r["category_id"] for r in recs] == [3, 7, 2]
    assert recs[0]["score"] == float(np.float32(0.9)) and recs[0]["segmentation"]["size"] == [11, 21]
    for r, (b, i) in zip(recs, [(0, 0), (0, 1), (1, 0)]):
        np.testing.assert_array_equal(CR.rle_decode(r["segmentation"]), planes[b][i])
    again = json.loads(json.dumps(recs))
    assert again == recs
    # the threshold is strict, the category map applies
    high = CR.coco_results([42, 7], det, rles, sizes, class_to_category={3: 30, 7: 70, 2: 20, 4: 40}, score_threshold=0.75)
    assert [(r["image_id"], r["category_id"]) for r in high] == [(42, 30)]
    assert CR.coco_results([42, 7], det, rles, sizes, score_threshold=float(np.float32(0.9))) == []


def test_the_entries_are_declared_listed_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "maskrcnn_hip.h")).read()
    lib_mod = _lib()
    for sym in NEW_SYMBOLS:
        assert re.search(r"MRCNN_API\s+int\s+%s\s*\(" % sym, hdr), sym
        assert sym in lib_mod.EXPORTED_SYMBOLS, sym
    assert os.path.exists(lib_mod.SO_PATH), "libmaskrcnn_hip.so not built (run python __graft_entry__.py)"
    raw = C.CDLL(lib_mod.SO_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), f"{sym} is not exported by libmaskrcnn_hip.so"
    assert len(lib_mod.lib().mrcnn_masks_rle_source.argtypes) == 17


def test_the_gpu_entry_has_no_cpu_fallback(pkg):
    """mrcnn_masks_rle_source computes on the GPU or not at all: MRCNN_ERR_HIP on a machine without one (and plain success with one)."""
    import torch
    lib = _lib()
    det = np.zeros((1, 2, 6), np.float32); det[0, 0] = [0.1, 0.1, 0.6, 0.6, 1, 0.9]
    masks = np.full((1, 2, 28, 28), 0.75, np.float32)
    hs = np.array([20], np.int32); ws = np.array([30], np.int32)
    src = np.zeros_like(det); counts = np.zeros(64, np.uint32); offs = np.zeros(3, np.int64)
    st = lib.lib().mrcnn_masks_rle_source(det.ctypes.data, masks.ctypes.data, 1, 2, 28, hs.ctypes.data, ws.ctypes.data, 64, 64, C.c_float(0.5),
                                          lib.HOST, src.ctypes.data, counts.ctypes.data, 64, offs.ctypes.data, None, None)
    if torch.cuda.is_available():
        assert st == 0, lib.lib().mrcnn_last_error()
        assert offs[0] == 0 and offs[2] == offs[1] + 1 and int(counts[:offs[1]].sum()) == 600 and counts[offs[1]] == 600
    else:
        assert st == 3, (st, lib.lib().mrcnn_last_error())
        with pytest.raises(lib.MrcnnError) as e:
            importlib.import_module("mask-rcnn-coreml_amd.detection").masks_rle_source(det, masks, [(20, 30)], 64, 64)
        assert e.value.code == 3
