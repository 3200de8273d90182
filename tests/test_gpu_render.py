"""Drawing detections on the GPU (mrcnn_instance_map_source, mrcnn_render_detections_source; detection.instance_map_source,
detection.render_detections_source, MaskRCNN.render_images).  Every comparison is bit for bit: the yardstick is the naive numpy
restatement of tests/test_render_host.py, fed with the planes of the oracle's numpy paste on the host-mapped boxes
(mrcnn_unletterbox_boxes) — the definition of mrcnn_paste_masks_source, which the entries are defined by."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_render_host import INC, ROOT, pixel_boxes, restate

gpu = pytest.mark.gpu

# widths that are no multiple of 4 or 16, a 2x5 image, a one-column image, h*w*3 and h*w*2 with every remainder mod 16
SIZES = [(37, 427), (250, 333), (3, 641), (480, 640), (2, 5), (7, 1), (96, 150)]
MODEL_H, MODEL_W = 256, 320
ROWS = 24
RENDER_CASES = [(128, 3), (256, 3), (0, 0), (77, 1), (128, 8)]               # (alpha, stroke)


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _D():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _blob(rng, S=28):
    """A smooth blob: a Gaussian bump somewhere in the mask, above 0.5 near its centre only."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    cy, cx = rng.uniform(8, 20, 2)
    sy, sx = rng.uniform(4, 9, 2)
    return np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)).astype(np.float32)


def _synthetic(sizes=SIZES, rows=ROWS, seed=31):
    """Detections in the LETTERBOXED frame of a 256x320 model and 28x28 masks in the style of test_gpu_mixed_batch.py::_synthetic:
    random boxes, scores in descending order from 0.99 down to 0.35 (the last third is at or below 0.7), odd rows random masks,
    even rows smooth blobs, plus that test's edge rows."""
    E = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
    rng = np.random.default_rng(seed)
    B = len(sizes)
    det = np.zeros((B, rows, 6), np.float32)
    masks = rng.random((B, rows, 28, 28)).astype(np.float32)
    for b, (h, w) in enumerate(sizes):
        nh, nw, py, px = E.letterbox_geometry(h, w, MODEL_H, MODEL_W)
        y1 = rng.random(rows) * 0.7; x1 = rng.random(rows) * 0.7
        det[b, :, 0] = y1; det[b, :, 1] = x1
        det[b, :, 2] = np.minimum(1.0, y1 + 0.02 + rng.random(rows) * 0.5); det[b, :, 3] = np.minimum(1.0, x1 + 0.02 + rng.random(rows) * 0.5)
        det[b, :, 4] = rng.integers(1, 80, rows)
        det[b, :, 5] = np.linspace(0.99, 0.35, rows)
        for i in range(0, rows, 2):
            masks[b, i] = _blob(rng)
        cy, cx = (py + nh // 2) / (MODEL_H - 1), (px + nw // 2) / (MODEL_W - 1)
        det[b, 3, :4] = [0, 0, 1, 1]                                        # the whole letterboxed frame: clipped to the whole image
        det[b, 4, :4] = [cy, cx, cy, cx]                                    # one-pixel box inside the content
        det[b, 5] = 0                                                       # padding row: stays all-zero, never drawn
        masks[b, 6] = 0.5                                                   # exactly on the threshold: kept (>=)
        # a box that lies partly in the letterbox border (from above / left of the content into it)
        det[b, 7, :4] = [max(0.0, (py - 9) / (MODEL_H - 1)), max(0.0, (px - 9) / (MODEL_W - 1)), (py + nh * 0.6) / (MODEL_H - 1), (px + nw * 0.6) / (MODEL_W - 1)]
        det[b, 8] = [0.2, 0.2, 0.6, 0.6, 9, 0.0]                            # score 0: never drawn, box still mapped
    return det, masks


def _sources(sizes=SIZES, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _expected_planes(det, masks, orc, thr, sizes=SIZES):
    L = _lib().lib()
    det_src = det.copy()
    planes = []
    for b, (h, w) in enumerate(sizes):
        _lib().check(L.mrcnn_unletterbox_boxes(det_src[b].ctypes.data, det.shape[1], 6, h, w, MODEL_H, MODEL_W))
        planes.append(orc.paste_masks(det_src[b], masks[b], h, w, thr))
    return det_src, planes


_CACHE = {}


def _case(orc):
    """(det, masks, det_src, planes, boxes) of the synthetic set, computed once per session."""
    if "case" not in _CACHE:
        det, masks = _synthetic()
        det_src, planes = _expected_planes(det, masks, orc, 0.5)
        boxes = [pixel_boxes(det_src[b], h, w) for b, (h, w) in enumerate(SIZES)]
        _CACHE["case"] = (det, masks, det_src, planes, boxes)
    return _CACHE["case"]


def _want(orc, b, min_score, stroke=0, alpha=128, src=None):
    det, masks, det_src, planes, boxes = _case(orc)
    return restate(boxes[b], det[b, :, 5], planes[b], min_score, stroke, alpha, src)


def test_the_inputs_have_teeth(pkg, orc):
    """Needs no GPU: the EXPECTED results exercise what the entries have to get right."""
    det, masks, det_src, planes, boxes = _case(orc)
    srcs = _sources()
    contested = winner_not_0 = ring_over_fill = ring_clipped = background = False
    for b, (h, w) in enumerate(SIZES):
        drawn = [i for i in range(ROWS) if det[b, i, 5] > 0 and boxes[b][i][2] > boxes[b][i][0]]
        assert 5 not in drawn and 8 not in drawn
        depth = planes[b][drawn].astype(np.int64).sum(0)
        contested |= (depth >= 2).mean() >= 0.01
        inst, visible, ring, _ = _want(orc, b, 0.0, stroke=3)
        assert int(visible.sum()) == int((inst >= 0).sum()) == int((depth > 0).sum())
        winner_not_0 |= bool((inst > 0).any())
        ring_over_fill |= bool(((ring >= 0) & (inst >= 0) & (inst != ring)).any())
        background |= bool(((inst < 0) & (ring < 0)).any())
        for i in drawn:                                                     # the grown box leaves the image and the ring is the winner there
            y1, x1, y2, x2 = boxes[b][i]
            if (y1 - 1 < 0 or x1 - 1 < 0 or y2 + 1 > h or x2 + 1 > w) and (ring == i).any():
                ring_clipped = True
    assert contested, "no image has two or more drawn planes on 1 % of its pixels"
    assert winner_not_0 and ring_over_fill and ring_clipped and background
    s = det[..., 5]
    assert ((s > 0) & (s <= np.float32(0.7))).any()
    changed = False
    for b in range(len(SIZES)):                                             # ... so that min_score changes the picture
        changed |= not np.array_equal(_want(orc, b, 0.0, 3, 128, srcs[b])[3], _want(orc, b, 0.7, 3, 128, srcs[b])[3])
    assert changed


@gpu
def test_the_map_is_the_lowest_drawn_plane(pkg, orc):
    D = _D()
    det, masks, want_src, planes, boxes = _case(orc)
    for min_score in (0.0, 0.7):
        det_src, maps, visible = D.instance_map_source(det, masks, SIZES, MODEL_H, MODEL_W, 0.5, min_score)
        np.testing.assert_array_equal(det_src, want_src)
        assert visible.shape == (len(SIZES), ROWS) and visible.dtype == np.uint32
        for b, (h, w) in enumerate(SIZES):
            inst, vis, _, _ = _want(orc, b, min_score)
            assert maps[b].shape == (h, w) and maps[b].dtype == np.int16
            np.testing.assert_array_equal(maps[b], inst, err_msg=f"map of image {b} {h}x{w}, min_score {min_score}")
            np.testing.assert_array_equal(visible[b], vis, err_msg=f"visible areas of image {b} {h}x{w}, min_score {min_score}")
    # the map derived from the GPU's own pasted planes is the same
    paste_src, pasted = D.paste_masks_source(det, masks, SIZES, MODEL_H, MODEL_W, 0.5)
    np.testing.assert_array_equal(paste_src, det_src)
    for b, (h, w) in enumerate(SIZES):
        np.testing.assert_array_equal(maps[b], restate(boxes[b], det[b, :, 5], pasted[b], 0.7)[0], err_msg=f"image {b}")
    # another threshold moves the planes and the map with them
    det8, planes8 = _expected_planes(det, masks, orc, 0.8)
    _, maps8, vis8 = D.instance_map_source(det, masks, SIZES, MODEL_H, MODEL_W, 0.8, 0.0)
    for b, (h, w) in enumerate(SIZES):
        inst, vis, _, _ = restate(boxes[b], det[b, :, 5], planes8[b], 0.0)
        np.testing.assert_array_equal(maps8[b], inst)
        np.testing.assert_array_equal(vis8[b], vis)


@gpu
@pytest.mark.parametrize("min_score", [0.0, 0.7])
@pytest.mark.parametrize("alpha,stroke", RENDER_CASES)
def test_the_render_is_the_restatement(pkg, orc, alpha, stroke, min_score):
    D = _D()
    det, masks, want_src, planes, boxes = _case(orc)
    srcs = _sources()
    keep = [s.copy() for s in srcs]
    out = D.render_detections_source(srcs, det, masks, MODEL_H, MODEL_W, 0.5, min_score, alpha, stroke)
    for b, (h, w) in enumerate(SIZES):
        want = _want(orc, b, min_score, stroke, alpha, srcs[b])[3]
        assert out[b].shape == (h, w, 3) and out[b].dtype == np.uint8
        np.testing.assert_array_equal(out[b], want, err_msg=f"image {b} {h}x{w}, alpha {alpha}, stroke {stroke}, min_score {min_score}")
        np.testing.assert_array_equal(srcs[b], keep[b])                     # the sources are read, never written


@gpu
def test_more_rows_than_one_cull_pass(pkg, orc):
    """600 rows: the block lists them in three passes of 256; the result is the restatement's all the same."""
    D = _D()
    sizes = [(61, 83), (40, 200)]
    det, masks = _synthetic(sizes, rows=600, seed=41)
    det[:, :, 5] = np.linspace(0.99, 0.2, 600)
    det[:, 5] = 0
    det[:, :300, 2] = np.minimum(det[:, :300, 2], det[:, :300, 0] + 0.08)   # the first half small, so that late rows still win pixels
    det[:, :300, 3] = np.minimum(det[:, :300, 3], det[:, :300, 1] + 0.08)
    det[:, 3] = det[:, 9]
    det_src, planes = _expected_planes(det, masks, orc, 0.5, sizes)
    srcs = _sources(sizes)
    got_src, maps, visible = D.instance_map_source(det, masks, sizes, MODEL_H, MODEL_W, 0.5, 0.0)
    out = D.render_detections_source(srcs, det, masks, MODEL_H, MODEL_W, 0.5, 0.3, 128, 3)
    np.testing.assert_array_equal(got_src, det_src)
    late = False
    for b, (h, w) in enumerate(sizes):
        boxes = pixel_boxes(det_src[b], h, w)
        inst, vis, _, _ = restate(boxes, det[b, :, 5], planes[b], 0.0)
        late |= bool((inst >= 256).any())
        np.testing.assert_array_equal(maps[b], inst)
        np.testing.assert_array_equal(visible[b], vis)
        np.testing.assert_array_equal(out[b], restate(boxes, det[b, :, 5], planes[b], 0.3, 3, 128, srcs[b])[3])
    assert late, "no pixel is won by a row of the second pass"


def _gapped(nbytes, front=48):
    offs, pos = [], front                                                   # a gap in front, a ragged gap after every image
    for n in nbytes:
        offs.append(pos)
        pos = (pos + n + 15) // 16 * 16 + 32
    return offs, pos


@gpu
@pytest.mark.parametrize("shift", [0, 6])
def test_the_map_on_the_device_leaves_the_gaps_alone(pkg, orc, shift):
    """Device buffers, gaps between the images, 0xAA everywhere first.  shift = 6: `map` itself is not 16-byte aligned."""
    import torch
    lib = _lib()
    det, masks, want_src, planes, boxes = _case(orc)
    nbytes = [2 * h * w for h, w in SIZES]
    offs, total = _gapped(nbytes)
    buf = torch.full((total + shift + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    out = buf[shift:]
    det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    src_g = torch.full(det.shape, -1.0, dtype=torch.float32, device="cuda")
    vis_g = torch.full((len(SIZES), ROWS), 77, dtype=torch.int32, device="cuda")
    hs = np.array([s[0] for s in SIZES], np.int32); ws = np.array([s[1] for s in SIZES], np.int32)
    offs_a = np.array(offs, np.int64)
    lib.check(lib.lib().mrcnn_instance_map_source(det_g.data_ptr(), masks_g.data_ptr(), len(SIZES), ROWS, 28, hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W,
                                                  C.c_float(0.5), C.c_float(0.7), lib.DEVICE, src_g.data_ptr(), out.data_ptr(), offs_a.ctypes.data, vis_g.data_ptr()))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(src_g.cpu().numpy(), want_src)
    covered = np.zeros(got.size, bool)
    for b, (h, w) in enumerate(SIZES):
        lo = shift + offs[b]
        inst, vis, _, _ = _want(orc, b, 0.7)
        np.testing.assert_array_equal(got[lo:lo + nbytes[b]].view(np.int16).reshape(h, w), inst, err_msg=f"image {b} {h}x{w}")
        np.testing.assert_array_equal(vis_g[b].cpu().numpy().view(np.uint32), vis)
        covered[lo:lo + nbytes[b]] = True
    assert (got[~covered] == 0xAA).all(), f"{int((got[~covered] != 0xAA).sum())} bytes outside the described maps were written"
    # the Python mirror on device tensors: used in place, torch tensors back; visible_areas = NULL is accepted
    src_t, maps_t, vis_t = _D().instance_map_source(det_g, masks_g, SIZES, MODEL_H, MODEL_W, 0.5, 0.7)
    assert src_t.is_cuda and vis_t.is_cuda and all(m.is_cuda for m in maps_t)
    for b in range(len(SIZES)):
        np.testing.assert_array_equal(maps_t[b].cpu().numpy(), _want(orc, b, 0.7)[0])
    buf.fill_(0xAA)
    lib.check(lib.lib().mrcnn_instance_map_source(det_g.data_ptr(), masks_g.data_ptr(), len(SIZES), ROWS, 28, hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W,
                                                  C.c_float(0.5), C.c_float(0.7), lib.DEVICE, src_g.data_ptr(), out.data_ptr(), offs_a.ctypes.data, None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), got)


@gpu
@pytest.mark.parametrize("shift", [0, 5])
def test_the_render_on_the_device_leaves_the_gaps_alone(pkg, orc, shift):
    """shift = 5: `out_rgb` itself is not 16-byte aligned (the kernel aligns its wide stores to the ADDRESS, so a lane's 48 bytes
    start inside a pixel); the third source image sits at an odd address too."""
    import torch
    lib = _lib()
    det, masks, want_src, planes, boxes = _case(orc)
    srcs = _sources()
    nbytes = [3 * h * w for h, w in SIZES]
    offs, total = _gapped(nbytes)
    buf = torch.full((total + shift + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    out = buf[shift:]
    det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    src_g = torch.full(det.shape, -1.0, dtype=torch.float32, device="cuda")
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    odd = torch.empty(nbytes[2] + 16, dtype=torch.uint8, device="cuda")
    odd[3:3 + nbytes[2]] = dev[2].reshape(-1)
    dev[2] = odd[3:3 + nbytes[2]].view(SIZES[2][0], SIZES[2][1], 3)
    table = (lib.Image * len(SIZES))()
    for b, t in enumerate(dev):
        table[b].rgb, table[b].height, table[b].width = t.data_ptr(), SIZES[b][0], SIZES[b][1]
    offs_a = np.array(offs, np.int64)
    for with_src in (True, False):
        buf.fill_(0xAA)
        lib.check(lib.lib().mrcnn_render_detections_source(table, det_g.data_ptr(), masks_g.data_ptr(), len(SIZES), ROWS, 28, MODEL_H, MODEL_W, C.c_float(0.5),
                                                           C.c_float(0.7), 128, 3, lib.DEVICE, src_g.data_ptr() if with_src else None, out.data_ptr(),
                                                           offs_a.ctypes.data))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        np.testing.assert_array_equal(src_g.cpu().numpy(), want_src)
        covered = np.zeros(got.size, bool)
        for b, (h, w) in enumerate(SIZES):
            lo = shift + offs[b]
            want = _want(orc, b, 0.7, 3, 128, srcs[b])[3]
            np.testing.assert_array_equal(got[lo:lo + nbytes[b]].reshape(h, w, 3), want, err_msg=f"image {b} {h}x{w}")
            covered[lo:lo + nbytes[b]] = True
            np.testing.assert_array_equal(dev[b].cpu().numpy(), srcs[b])
        assert (got[~covered] == 0xAA).all(), f"{int((got[~covered] != 0xAA).sum())} bytes outside the described images were written"
    # the Python mirror on device tensors
    out_t = _D().render_detections_source(dev, det_g, masks_g, MODEL_H, MODEL_W)
    for b in range(len(SIZES)):
        assert out_t[b].is_cuda
        np.testing.assert_array_equal(out_t[b].cpu().numpy(), _want(orc, b, 0.7, 3, 128, srcs[b])[3])


@gpu
def test_bad_arguments_are_refused(pkg):
    lib = _lib()
    L = lib.lib()
    INVALID, SHAPE = 1, 4
    det, masks = _synthetic(rows=12)
    sizes = SIZES[:5]
    B, rows = len(sizes), 12
    det, masks = det[:B], masks[:B]
    hs = np.array([s[0] for s in sizes], np.int32); ws = np.array([s[1] for s in sizes], np.int32)
    srcs = _sources(sizes)
    src = np.zeros_like(det)
    out = np.zeros(8 << 20, np.uint8)
    vis = np.zeros((B, rows), np.uint32)
    good = [0, 1 << 20, 2 << 20, 3 << 20, 7 << 20]                          # (the largest image: 480 x 640 x 3 = 0.9 MB)

    def map_call(hs=hs, ws=ws, offs=good, rows=rows, det_p=det.ctypes.data, masks_p=masks.ctypes.data, src_p=src.ctypes.data, out_p=out.ctypes.data,
                 null_offs=False, null_sizes=False):
        offs = np.array(offs, np.int64)
        st = L.mrcnn_instance_map_source(det_p, masks_p, B, rows, 28, None if null_sizes else hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W, C.c_float(0.5),
                                         C.c_float(0.0), lib.HOST, src_p, out_p, None if null_offs else offs.ctypes.data, vis.ctypes.data)
        return st, L.mrcnn_last_error().decode(errors="replace")

    def table_of(entries):
        t = (lib.Image * len(entries))()
        for i, (p, h, w) in enumerate(entries):
            t[i].rgb, t[i].height, t[i].width = p, h, w
        return t
    ok = [(im.ctypes.data, im.shape[0], im.shape[1]) for im in srcs]

    def render_call(entries=ok, offs=good, rows=rows, alpha=128, stroke=3, det_p=det.ctypes.data, masks_p=masks.ctypes.data, out_p=out.ctypes.data,
                    null_table=False, null_offs=False):
        offs = np.array(offs, np.int64)
        st = L.mrcnn_render_detections_source(None if null_table else table_of(entries), det_p, masks_p, B, rows, 28, MODEL_H, MODEL_W, C.c_float(0.5),
                                              C.c_float(0.7), alpha, stroke, lib.HOST, None, out_p, None if null_offs else offs.ctypes.data)
        return st, L.mrcnn_last_error().decode(errors="replace")

    assert map_call()[0] == 0 and render_call()[0] == 0
    # null pointers
    for kw in ({"det_p": None}, {"masks_p": None}, {"src_p": None}, {"out_p": None}, {"null_offs": True}, {"null_sizes": True}):
        st, msg = map_call(**kw)
        assert st == INVALID and "null" in msg, (kw, st, msg)
    for kw in ({"det_p": None}, {"masks_p": None}, {"out_p": None}, {"null_offs": True}, {"null_table": True}):
        st, msg = render_call(**kw)
        assert st == INVALID and "null" in msg, (kw, st, msg)
    bad = list(ok); bad[1] = (None, ok[1][1], ok[1][2])                     # a null rgb in slot 1
    st, msg = render_call(entries=bad)
    assert st == INVALID and "image 1" in msg, (st, msg)
    # sizes
    bad_h = hs.copy(); bad_h[2] = 0
    st, msg = map_call(hs=bad_h)
    assert st == SHAPE and "image 2" in msg, (st, msg)
    bad_w = ws.copy(); bad_w[3] = 32768
    st, msg = map_call(ws=bad_w)
    assert st == SHAPE and "image 3" in msg, (st, msg)
    bad = list(ok); bad[2] = (ok[2][0], 0, ok[2][2])
    st, msg = render_call(entries=bad)
    assert st == SHAPE and "image 2" in msg, (st, msg)
    bad = list(ok); bad[4] = (ok[4][0], 2, 32768)
    st, msg = render_call(entries=bad)
    assert st == SHAPE and "image 4" in msg, (st, msg)
    # rows above what the int16 map holds (refused before anything is read)
    st, msg = map_call(rows=32768)
    assert st == SHAPE and "32768 rows" in msg, (st, msg)
    st, msg = render_call(rows=32768)
    assert st == SHAPE and "32768 rows" in msg, (st, msg)
    # alpha and stroke
    for a in (-1, 257):
        st, msg = render_call(alpha=a)
        assert st == SHAPE and "alpha" in msg, (a, st, msg)
    st, msg = render_call(stroke=-1)
    assert st == SHAPE and "stroke" in msg, (st, msg)
    # offsets
    for call in (map_call, render_call):
        st, msg = call(offs=[0, (1 << 20) + 4, 2 << 20, 3 << 20, 7 << 20])  # not a multiple of 16
        assert st == INVALID and "image 1" in msg, (st, msg)
        st, msg = call(offs=[0, 16, 2 << 20, 3 << 20, 7 << 20])             # image 1 inside image 0
        assert st == INVALID and "overlap" in msg, (st, msg)
        st, msg = call(offs=[0, -16, 2 << 20, 3 << 20, 7 << 20])
        assert st == INVALID and "image 1" in msg, (st, msg)
    assert map_call()[0] == 0 and render_call()[0] == 0                     # and the entries still work


@gpu
def test_render_images_end_to_end(pkg, small_model):
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(96, 160), (300, 200), (37, 53), (128, 128)]]
    det, mask = m.predict_images(images)
    assert (det[..., 5] > 0.7).any(), "no detection above 0.7: nothing is drawn"
    want = _D().render_detections_source(images, det, mask, m.image_height, m.image_width)
    got = m.render_images(images)
    assert len(got) == 4 and any(not np.array_equal(g, im) for g, im in zip(got, images))
    for b in range(4):
        np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b}")
        one = m.render_images([images[b]])                                  # a batch of one is its row of the batch
        np.testing.assert_array_equal(one[0], got[b], err_msg=f"image {b} alone")
    # keyword arguments reach the render
    opaque = m.render_images(images, alpha=256, stroke=0, min_score=0.0)
    want = _D().render_detections_source(images, det, mask, m.image_height, m.image_width, 0.5, 0.0, 256, 0)
    for b in range(4):
        np.testing.assert_array_equal(opaque[b], want[b])


@gpu
def test_the_plain_c_host_writes_the_mirrors_picture(pkg, small_model, tmp_path):
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    libdir = os.path.dirname(_lib().SO_PATH)
    exe = str(tmp_path / "maskrcnn_render")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, os.path.join(ROOT, "examples", "maskrcnn_render.c"),
                        "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d, cfg = small_model
    img = np.random.default_rng(21).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    (tmp_path / "img.rgb").write_bytes(img.tobytes())
    env = {k: v for k, v in os.environ.items() if k != "MRCNN_TEST_KNOBS"}     # a production process
    r = subprocess.run([exe, d, str(tmp_path / "img.rgb"), "100", "150", str(tmp_path / "out.ppm")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    drawn = int(r.stdout.split()[1])
    blob = (tmp_path / "out.ppm").read_bytes()
    head = b"P6\n150 100\n255\n"
    assert blob.startswith(head) and len(blob) == len(head) + 100 * 150 * 3
    got = np.frombuffer(blob[len(head):], np.uint8).reshape(100, 150, 3)
    m = models.load_maskrcnn(d, max_batch=1)                                # the mirror names no precision either
    det, _ = m.predict_images([img])
    assert drawn == int((det[0, :, 5] > np.float32(0.7)).sum()) and drawn > 0
    want = m.render_images([img])[0]
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, img)
