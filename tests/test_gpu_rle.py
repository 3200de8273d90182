"""COCO run-length encoding on the GPU (mrcnn_masks_rle_source, detection.masks_rle_source, evaluate.evaluate_segm): for every image
and row the encoded mask IS the plane mrcnn_paste_masks_source pastes — and the plane of the oracle's numpy paste on the
host-mapped boxes, so the yardstick is not only the project's own kernel — with maximal runs, plus area and tight box.  Every
comparison is exact."""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the size family of test_gpu_mixed_batch.py's paste tests, plus a 1 x N and an N x 1 image
PASTE_SIZES = [(37, 427), (250, 333), (3, 641), (480, 640), (7, 1), (1, 97), (211, 1)]
MODEL_H, MODEL_W = 256, 320
GUARD = 0x5A5A5A5A


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _blob(rng):
    """A smooth 28x28 mask as a network draws it: a few long runs per column."""
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    cy, cx = rng.uniform(8, 20, 2)
    sy, sx = rng.uniform(4, 12, 2)
    return np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)).astype(np.float32)


def _synthetic(rows=24, seed=21):
    """test_gpu_mixed_batch.py's _synthetic (random boxes in the LETTERBOXED frame of a 256x320 model, uniform-random masks: many
    runs per column, and its edge rows 3..8), restated; every odd row from 15 on carries a smooth blob instead, and rows 9..14 are:
       9   full image height, a band of columns, everything above the threshold: every column joins the next — ONE run of ones
       10  the same box, only the top and the bottom rows of the mask set: each run leaves a column at the bottom edge and enters
           the next at the top
       11  the whole image, everything above the threshold: [0, h*w]
       12  the whole image, a blob
       13  from the top edge down to the middle (touches only the top), random
       14  from the middle to the bottom edge (touches only the bottom), random"""
    E = _mod("evaluate")
    rng = np.random.default_rng(seed)
    B = len(PASTE_SIZES)
    det = np.zeros((B, rows, 6), np.float32)
    masks = rng.random((B, rows, 28, 28)).astype(np.float32)
    for b, (h, w) in enumerate(PASTE_SIZES):
        nh, nw, py, px = E.letterbox_geometry(h, w, MODEL_H, MODEL_W)
        y1 = rng.random(rows) * 0.7; x1 = rng.random(rows) * 0.7
        det[b, :, 0] = y1; det[b, :, 1] = x1
        det[b, :, 2] = np.minimum(1.0, y1 + 0.02 + rng.random(rows) * 0.5); det[b, :, 3] = np.minimum(1.0, x1 + 0.02 + rng.random(rows) * 0.5)
        det[b, :, 4] = rng.integers(1, 80, rows); det[b, :, 5] = 0.7 + 0.3 * rng.random(rows)
        det[b, 3] = [0, 0, 1, 1, 5, 0.99]                                   # the whole letterboxed frame: clipped to the whole image
        cy, cx = (py + nh // 2) / (MODEL_H - 1), (px + nw // 2) / (MODEL_W - 1)
        det[b, 4] = [cy, cx, cy, cx, 5, 0.9]                                # one-pixel box inside the content
        det[b, 5] = 0                                                       # padding row: stays all-zero, empty mask
        masks[b, 6] = 0.5                                                   # exactly on the threshold: kept (>=)
        det[b, 7] = [max(0.0, (py - 9) / (MODEL_H - 1)), max(0.0, (px - 9) / (MODEL_W - 1)), (py + nh * 0.6) / (MODEL_H - 1), (px + nw * 0.6) / (MODEL_W - 1), 7, 0.8]
        det[b, 8] = [0.2, 0.2, 0.6, 0.6, 9, 0.0]                            # score 0: empty mask, box still mapped
        xa, xb = (px + nw * 0.25) / (MODEL_W - 1), (px + nw * 0.7) / (MODEL_W - 1)
        ym = (py + nh * 0.5) / (MODEL_H - 1)
        det[b, 9] = [0, xa, 1, xb, 11, 0.95]; masks[b, 9] = 0.9
        det[b, 10] = [0, xa, 1, xb, 12, 0.95]; masks[b, 10] = 0.1; masks[b, 10, :5] = 0.9; masks[b, 10, -5:] = 0.9
        det[b, 11] = [0, 0, 1, 1, 13, 0.95]; masks[b, 11] = 0.9
        det[b, 12] = [0, 0, 1, 1, 14, 0.95]; masks[b, 12] = _blob(rng)
        det[b, 13] = [0, xa, ym, xb, 15, 0.95]
        det[b, 14] = [ym, xa, 1, xb, 16, 0.95]
        for i in range(15, rows, 2):
            masks[b, i] = _blob(rng)
    return det, masks


def _oracle_planes(det, masks, orc, thr):
    lib = _mod("_lib")
    det_src = det.copy()
    planes = []
    for b, (h, w) in enumerate(PASTE_SIZES):
        lib.check(lib.lib().mrcnn_unletterbox_boxes(det_src[b].ctypes.data, det.shape[1], 6, h, w, MODEL_H, MODEL_W))
        planes.append(orc.paste_masks(det_src[b], masks[b], h, w, thr))
    return det_src, planes


def _tight(plane):
    ys, xs = np.nonzero(plane)
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def _check_against_planes(rles, areas, bboxes, planes, rows, tag):
    CR = _mod("coco_results")
    for b, (h, w) in enumerate(PASTE_SIZES):
        for i in range(rows):
            rle, plane = rles[b][i], planes[b][i]
            where = f"{tag}: image {b} {h}x{w} row {i}"
            assert rle["size"] == [h, w], where
            c = np.asarray(rle["counts"])
            assert c.dtype == np.uint32 and int(c.astype(np.int64).sum()) == h * w, where
            np.testing.assert_array_equal(CR.rle_decode(rle), plane, err_msg=where)
            np.testing.assert_array_equal(c, CR.rle_encode(plane)["counts"], err_msg=where)      # maximal runs, none split at a column
            assert int(areas[b, i]) == int(plane.sum()), where
            assert [int(v) for v in bboxes[b, i]] == _tight(plane), where


def test_rle_is_the_pasted_plane(pkg, orc):
    D = _mod("detection")
    det, masks = _synthetic()
    rows = det.shape[1]
    assert any(w % 4 for _, w in PASTE_SIZES)
    want_src, want = _oracle_planes(det, masks, orc, 0.5)
    paste_src, pasted = D.paste_masks_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    det_src, rles, areas, bboxes = D.masks_rle_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    np.testing.assert_array_equal(det_src, paste_src)
    np.testing.assert_array_equal(det_src, want_src)
    assert areas.shape == (len(PASTE_SIZES), rows) and bboxes.shape == (len(PASTE_SIZES), rows, 4)
    _check_against_planes(rles, areas, bboxes, pasted, rows, "paste_masks_source")
    _check_against_planes(rles, areas, bboxes, want, rows, "oracle")
    # the cases are what they claim to be
    many = one_pixel = 0
    for b, (h, w) in enumerate(PASTE_SIZES):
        np.testing.assert_array_equal(rles[b][5]["counts"], [h * w])                      # the padding row
        np.testing.assert_array_equal(rles[b][8]["counts"], [h * w])                      # score 0
        np.testing.assert_array_equal(rles[b][11]["counts"], [0, h * w])                  # the whole image set
        np.testing.assert_array_equal(rles[b][3]["counts"], [0, h * w] if (masks[b, 3] >= 0.5).all() else rles[b][3]["counts"])
        r4 = det_src[b, 4].astype(np.float64)                                             # one pixel of the letterboxed frame
        px4 = (int(np.rint(r4[2] * (h - 1) + 1.0)) - int(np.rint(r4[0] * (h - 1)))) * (int(np.rint(r4[3] * (w - 1) + 1.0)) - int(np.rint(r4[1] * (w - 1))))
        assert int(areas[b, 4]) <= px4
        one_pixel += int(px4 == 1)
        assert len(rles[b][9]["counts"]) <= 3 and int(areas[b, 9]) % h == 0 and int(areas[b, 9]) > 0     # whole columns joined into ONE run
        if h >= 28:                         # top and bottom set, the middle not: a column's bottom run and the next column's top run are
            bw = int(bboxes[b, 10, 2])      # ONE run — bw + 1 runs of ones for bw columns, not 2 bw
            assert bw >= 1 and int(bboxes[b, 10, 3]) == h and len(rles[b][10]["counts"][1::2]) == bw + 1, (b, bw, len(rles[b][10]["counts"]))
        many = max(many, max(len(rles[b][i]["counts"]) for i in range(rows)))
    assert one_pixel > 0                                                                  # ... a one-pixel box in the image's own pixels among them
    assert many > 2000, many                                                              # the random masks really give many runs


def test_device_buffers_guards_capacity_and_query(pkg, orc):
    import torch
    D = _mod("detection")
    lib = _mod("_lib")
    L = lib.lib()
    det, masks = _synthetic(rows=16, seed=22)
    B, rows = det.shape[0], det.shape[1]
    n = B * rows
    host_src, host_rles, host_areas, host_boxes = D.masks_rle_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    flat = np.concatenate([r["counts"] for per in host_rles for r in per])
    offs_want = np.concatenate(([0], np.cumsum([len(r["counts"]) for per in host_rles for r in per]))).astype(np.int64)
    need = int(offs_want[-1])
    hs = np.array([s[0] for s in PASTE_SIZES], np.int32); ws = np.array([s[1] for s in PASTE_SIZES], np.int32)
    det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    PAD = 64

    def fresh():
        i32 = lambda k: torch.full((k,), GUARD, dtype=torch.int32, device="cuda")
        return {"src": torch.full((n * 6 + PAD,), -7.0, dtype=torch.float32, device="cuda"), "counts": i32(need + PAD),
                "offs": torch.full((n + 1 + PAD,), GUARD, dtype=torch.int64, device="cuda"), "areas": i32(n + PAD), "boxes": i32(4 * n + PAD)}

    def call(buf, capacity, counts_ptr=True, det_ptr=None, heights=hs, widths=ws, batch=B, nrows=rows, S=28):
        st = L.mrcnn_masks_rle_source(det_g.data_ptr() if det_ptr is None else det_ptr, masks_g.data_ptr(), batch, nrows, S, heights.ctypes.data,
                                      widths.ctypes.data, MODEL_H, MODEL_W, C.c_float(0.5), lib.DEVICE, buf["src"].data_ptr(),
                                      buf["counts"].data_ptr() if counts_ptr else None, capacity, buf["offs"].data_ptr(), buf["areas"].data_ptr(),
                                      buf["boxes"].data_ptr())
        torch.cuda.synchronize()
        return st, L.mrcnn_last_error().decode(errors="replace")

    def outputs_ok(buf):
        np.testing.assert_array_equal(buf["src"].cpu().numpy()[:n * 6].reshape(det.shape), host_src)
        np.testing.assert_array_equal(buf["offs"].cpu().numpy()[:n + 1], offs_want)
        np.testing.assert_array_equal(buf["areas"].cpu().numpy()[:n].view(np.uint32).reshape(B, rows), host_areas)
        np.testing.assert_array_equal(buf["boxes"].cpu().numpy()[:4 * n].reshape(B, rows, 4), host_boxes)
        assert (buf["src"].cpu().numpy()[n * 6:] == -7.0).all()
        assert (buf["offs"].cpu().numpy()[n + 1:] == GUARD).all()
        assert (buf["areas"].cpu().numpy()[n:] == GUARD).all() and (buf["boxes"].cpu().numpy()[4 * n:] == GUARD).all()

    # exactly the capacity needed: the same runs as the host call, nothing behind any output
    buf = fresh()
    st, msg = call(buf, need)
    assert st == 0, msg
    outputs_ok(buf)
    got = buf["counts"].cpu().numpy()
    np.testing.assert_array_equal(got[:need].view(np.uint32), flat)
    assert (got[need:] == GUARD).all()
    # the Python entry on device tensors: the same, results left on the device
    src_t, rles_t, areas_t, boxes_t = D.masks_rle_source(det_g, masks_g, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    assert src_t.is_cuda and areas_t.is_cuda and boxes_t.is_cuda
    np.testing.assert_array_equal(src_t.cpu().numpy(), host_src)
    np.testing.assert_array_equal(areas_t.cpu().numpy().view(np.uint32), host_areas)
    np.testing.assert_array_equal(boxes_t.cpu().numpy(), host_boxes)
    for b in range(B):
        for i in range(rows):
            np.testing.assert_array_equal(rles_t[b][i]["counts"], host_rles[b][i]["counts"])
    # one short: MRCNN_ERR_SHAPE, the needed capacity in the message, everything else complete, counts[capacity:] untouched
    buf = fresh()
    st, msg = call(buf, need - 1)
    assert st == 4 and str(need) in msg, (st, msg)
    outputs_ok(buf)
    assert (buf["counts"].cpu().numpy()[need - 1:] == GUARD).all()
    buf = fresh()
    st, msg = call(buf, 5)
    assert st == 4 and str(need) in msg, (st, msg)
    outputs_ok(buf)
    assert (buf["counts"].cpu().numpy()[5:] == GUARD).all()
    # the query form
    buf = fresh()
    st, msg = call(buf, 0, counts_ptr=False)
    assert st == 4 and str(need) in msg, (st, msg)
    outputs_ok(buf)
    assert (buf["counts"].cpu().numpy() == GUARD).all()
    # bad arguments: the paste entry's status codes
    buf = fresh()
    assert call(buf, need, det_ptr=0)[0] == 1                                # a null pointer: MRCNN_ERR_INVALID
    assert call(buf, need, counts_ptr=False)[0] == 1                         # null counts with a capacity
    assert call(buf, -1)[0] == 1
    assert call(buf, need, S=1)[0] == 1
    bad_h = hs.copy(); bad_h[2] = 0
    st, msg = call(buf, need, heights=bad_h)
    assert st == 4 and "image 2" in msg, (st, msg)
    bad_w = ws.copy(); bad_w[1] = 32768
    st, msg = call(buf, need, widths=bad_w)
    assert st == 4 and "image 1" in msg, (st, msg)
    assert call(buf, need, batch=65536, nrows=32768)[0] == 4                 # batch * rows >= 2^31 (refused before anything is read)
    outputs_unwritten = fresh()
    for k in buf:
        np.testing.assert_array_equal(buf[k].cpu().numpy(), outputs_unwritten[k].cpu().numpy())      # a refused call writes nothing
    # ... and the call after the refused ones works
    st, msg = call(buf, need + 7)
    assert st == 0, msg
    outputs_ok(buf)
    got = buf["counts"].cpu().numpy()
    np.testing.assert_array_equal(got[:need].view(np.uint32), flat)
    assert (got[need:] == GUARD).all()
    # areas / bboxes_xywh may be NULL; an empty batch still writes run_offsets[0]
    st = L.mrcnn_masks_rle_source(det_g.data_ptr(), masks_g.data_ptr(), B, rows, 28, hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W, C.c_float(0.5),
                                  lib.DEVICE, buf["src"].data_ptr(), buf["counts"].data_ptr(), need, buf["offs"].data_ptr(), None, None)
    assert st == 0
    np.testing.assert_array_equal(buf["counts"].cpu().numpy()[:need].view(np.uint32), flat)
    buf = fresh()
    assert call(buf, 0, batch=0)[0] == 0
    assert buf["offs"].cpu().numpy()[0] == 0 and (buf["offs"].cpu().numpy()[1:] == GUARD).all()


def test_two_calls_give_identical_counts(pkg):
    D = _mod("detection")
    det, masks = _synthetic(rows=24, seed=23)
    a = D.masks_rle_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    b = D.masks_rle_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[2], b[2]); np.testing.assert_array_equal(a[3], b[3])
    for ra, rb in zip(a[1], b[1]):
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x["counts"], y["counts"])
    # another threshold is another answer (the threshold reaches the kernel)
    c = D.masks_rle_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.8)
    assert int(c[2].sum()) < int(a[2].sum())


@pytest.mark.parametrize("mode", ["f32x3", "f16"])
def test_evaluate_segm_end_to_end(pkg, small_model, mode):
    E, D, CR = _mod("evaluate"), _mod("detection"), _mod("coco_results")
    d, cfg = small_model
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype=mode)
    sizes = [(96, 160), (300, 200), (128, 128), (37, 53), (64, 427), (333, 100), (200, 201)]
    rng = np.random.default_rng(11)
    items = [(50 - i, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for i, (h, w) in enumerate(sizes)]
    blob, secs, recs, coco = E.evaluate_segm(m, items, limit=None, verbose=False, batch=4)
    blob1, _, _ = E.evaluate(m, items, limit=None, verbose=False, batch=1)
    assert blob == blob1 and len(secs) == 7 and len(recs) == 7                 # results.proto: the bytes of the batch-1 loop, as before
    assert blob == E.evaluate(m, items, limit=None, verbose=False, batch=4)[0]
    json.dumps(coco)
    # the expectation: the same images through the host path, pasted
    by_id = sorted(items, key=lambda it: it[0])
    k = 0
    teeth = 0
    for g0 in range(0, 7, 4):
        group = by_id[g0:g0 + 4]
        gs = [im.shape[:2] for _, im in group]
        det, mask = m.predict_images([im for _, im in group])
        det_src, planes = D.paste_masks_source(det, mask, gs, cfg.image_height, cfg.image_width, 0.5)
        for b, (image_id, im) in enumerate(group):
            h, w = gs[b]
            for i in range(det.shape[1]):
                if not det_src[b, i, 5] > 0:
                    continue
                r = coco[k]; k += 1
                assert r["image_id"] == image_id and r["category_id"] == int(det_src[b, i, 4]) and r["score"] == float(det_src[b, i, 5])
                assert r["segmentation"]["size"] == [h, w] and isinstance(r["segmentation"]["counts"], str)
                np.testing.assert_array_equal(CR.rle_decode(r["segmentation"]), planes[b][i], err_msg=f"{mode}: image {image_id} row {i}")
                y1, x1 = int(np.rint(float(det_src[b, i, 0]) * (h - 1))), int(np.rint(float(det_src[b, i, 1]) * (w - 1)))
                y2, x2 = int(np.rint(float(det_src[b, i, 2]) * (h - 1) + 1.0)), int(np.rint(float(det_src[b, i, 3]) * (w - 1) + 1.0))
                assert r["bbox"] == [x1, y1, x2 - x1, y2 - y1]
                teeth += int(0 < int(planes[b][i].sum()) < h * w)
    assert k == len(coco) and k > 0
    assert teeth > 0, "no detection with a non-empty, non-full mask: the comparison has no teeth"
