"""Mixed-size batches on the GPU: MaskRCNN.predict_images (mrcnn_maskrcnn_predict_images — one predict over images of different
sizes, each letterboxed with its own geometry inside the one pre-processing launch) and paste_masks_source
(mrcnn_paste_masks_source — boxes and binary masks in every image's own pixels, any width).  Every comparison is bit for bit:
the reference of predict_images is predict_scalefit on each image alone (the engine's batch independence is pinned by
test_gpu_fullsize.py), the reference of the paste is the oracle's numpy restatement on the host-mapped boxes."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import make_model_dir, rand_images

pytestmark = pytest.mark.gpu

SIZES = [(96, 160), (300, 200), (128, 128), (37, 53), (2, 5), (640, 427)]


def _models():
    return importlib.import_module("mask-rcnn-coreml_amd.models")


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _mixed(sizes, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _one_by_one(m, images):
    """The reference: every image through predict_scalefit in a call of its own."""
    rows = [m.predict_scalefit(im[None]) for im in images]
    return np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])


@pytest.mark.parametrize("mode", ["f32x3", "f32", "f32s", "f16"])
def test_a_mixed_batch_equals_each_image_alone(pkg, small_model, mode):
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=6, compute_dtype=mode)
    images = _mixed(SIZES)
    det, mask = m.predict_images(images)
    assert det.shape == (6, m.max_detections, 6) and mask.shape == (6, m.max_detections, m.mask_size, m.mask_size)
    want_d, want_m = _one_by_one(m, images)
    assert (want_d[..., 5] > 0).any(), "no detection at all: the comparison has no teeth"
    for b in range(6):
        np.testing.assert_array_equal(det[b], want_d[b], err_msg=f"{mode}: detections of image {b} {SIZES[b]}")
        np.testing.assert_array_equal(mask[b], want_m[b], err_msg=f"{mode}: masks of image {b} {SIZES[b]}")


def test_one_size_a_permutation_a_batch_of_one_and_no_state_left(pkg, small_model):
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=6, compute_dtype="f32x3")
    plain = rand_images(2, cfg.image_height, cfg.image_width, seed=4)
    before = m.predict(plain)
    # six images of ONE size: the stacked array through predict_scalefit
    same = rand_images(6, 200, 150, seed=5)
    det, mask = m.predict_images(list(same))
    want_d, want_m = m.predict_scalefit(same)
    np.testing.assert_array_equal(det, want_d)
    np.testing.assert_array_equal(mask, want_m)
    # a permutation of the batch permutes the results
    images = _mixed(SIZES)
    det, mask = m.predict_images(images)
    perm = [4, 0, 5, 2, 1, 3]
    det_p, mask_p = m.predict_images([images[i] for i in perm])
    np.testing.assert_array_equal(det_p, det[perm])
    np.testing.assert_array_equal(mask_p, mask[perm])
    # a batch of one
    d1, m1 = m.predict_images([images[1]])
    np.testing.assert_array_equal(d1[0], det[1])
    np.testing.assert_array_equal(m1[0], mask[1])
    # a plain predict afterwards sees no state of the mixed path; nor does predict_scalefit
    after = m.predict(plain)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    s_d, s_m = m.predict_scalefit(images[5][None])
    np.testing.assert_array_equal(s_d[0], det[5])
    np.testing.assert_array_equal(s_m[0], mask[5])


@pytest.mark.parametrize("mode", ["f32x3", "f16"])
def test_device_images_equal_the_host_run(pkg, small_model, mode):
    import torch
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=6, compute_dtype=mode)
    images = _mixed(SIZES)
    det, mask = m.predict_images(images)
    dev = [torch.from_numpy(im).cuda() for im in images]
    det_g, mask_g = m.predict_images(dev)
    assert det_g.is_cuda and mask_g.is_cuda
    np.testing.assert_array_equal(det_g.cpu().numpy(), det)
    np.testing.assert_array_equal(mask_g.cpu().numpy(), mask)
    for t, im in zip(dev, images):                     # the caller's images are read, never written
        np.testing.assert_array_equal(t.cpu().numpy(), im)


def _rescaled_model(tmp_path_factory, pkg, weights_mod, name):
    """The small synthetic model made positively homogeneous (every trunk bias, BatchNorm beta and BatchNorm mean zeroed: conv →
    scale → ReLU only; the RPN heads keep their biases) — the model of test_gpu_split_scale.py's recovery test: its activations
    scale with the input's distance from the mean pixel, so a calibration on a nearly mean-coloured image leaves every real image
    far above the calibrated range."""
    d, cfg = make_model_dir(tmp_path_factory, pkg, weights_mod, name, architecture="resnet50", input_image_shape=(128, 128, 3),
                            num_classes=21, pre_nms_max_proposals=300, max_proposals=64, max_detections=16)
    path = os.path.join(d, "MaskRCNN.mrcw")
    meta, t = weights_mod.read_mrcw(path)
    t = dict(t)
    for k in list(t):
        if k.endswith("/beta") or k.endswith("/mean") or (k.endswith("/bias") and not k.startswith(("rpn_class_raw", "rpn_bbox_pred"))):
            t[k] = np.zeros_like(t[k])
    weights_mod.write_mrcw(path, meta, t)
    return d, cfg


def test_a_mixed_batch_above_the_calibrated_range_recovers(pkg, weights_mod, tmp_path_factory):
    """Range recovery of the split modes inside a mixed batch: the batch is measured and computed again from the sources and the
    geometry table still resident on the device.  A legitimate input above the calibrated range, once (the way
    test_gpu_split_scale.py provokes it)."""
    d, cfg = _rescaled_model(tmp_path_factory, pkg, weights_mod, "recover_mixed")
    flat = np.empty((1, 128, 128, 3), np.uint8)
    flat[...] = np.array([124, 117, 104], np.uint8)                         # mean pixel (123.7, 116.8, 103.9) + < 1
    sizes = [(96, 160), (300, 200), (37, 53)]
    images = _mixed(sizes, seed=9)
    m = _models().load_maskrcnn(d, max_batch=3, compute_dtype="f32x3")
    m.calibrate_split(flat)
    hi = int(m.get_int("split_max_exponent"))
    assert hi >= 12, hi                                                     # the calibration image really was tiny
    r0 = m.get_int("range_recoveries")
    det, mask = m.predict_images(images)                                    # succeeds
    assert m.get_int("range_recoveries") == r0 + 1
    assert int(m.get_int("split_max_exponent")) < hi
    # a second handle given the recovered exponents reproduces every image's record, one image per call
    m2 = _models().load_maskrcnn(d, max_batch=1, compute_dtype="f32x3")
    m2.split_exponents = m.split_exponents
    for b, im in enumerate(images):
        d1, m1 = m2.predict_scalefit(im[None])
        np.testing.assert_array_equal(d1[0], det[b], err_msg=f"image {b}")
        np.testing.assert_array_equal(m1[0], mask[b], err_msg=f"image {b}")
    assert m2.get_int("range_recoveries") == 0
    assert (det[..., 5] > 0).any()


def _raw_predict_images(m, entries, batch=None, null_table=False):
    """The C entry with a hand-made table: entries = [(pointer or None, h, w)].  Returns (status, message, det, mask)."""
    lib = _lib()
    L = lib.lib()
    B = len(entries) if batch is None else batch
    table = (lib.Image * max(1, len(entries)))()
    for i, (ptr, h, w) in enumerate(entries):
        table[i].rgb, table[i].height, table[i].width = ptr, h, w
    det = np.zeros((max(1, len(entries)), m.max_detections, 6), np.float32)
    mask = np.zeros((max(1, len(entries)), m.max_detections, m.mask_size, m.mask_size), np.float32)
    st = L.mrcnn_maskrcnn_predict_images(m._h, None if null_table else table, B, lib.HOST, det.ctypes.data, mask.ctypes.data)
    return st, L.mrcnn_last_error().decode(errors="replace"), det, mask


def test_errors_name_the_image_and_leave_the_handle_usable(pkg, small_model):
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    images = _mixed([(96, 160), (300, 200), (37, 53), (64, 64), (50, 70)])
    want_d, want_m = m.predict_images(images[:4])
    ok = [(im.ctypes.data, im.shape[0], im.shape[1]) for im in images]

    def still_correct():
        det, mask = m.predict_images(images[:4])
        np.testing.assert_array_equal(det, want_d)
        np.testing.assert_array_equal(mask, want_m)

    INVALID, SHAPE = 1, 4
    st, msg, _, _ = _raw_predict_images(m, ok)                              # batch = max_batch + 1
    assert st == SHAPE and "batch 5" in msg, (st, msg)
    still_correct()
    st, msg, _, _ = _raw_predict_images(m, ok[:4], batch=0)
    assert st == SHAPE, (st, msg)
    bad = list(ok[:4]); bad[1] = (ok[1][0], 0, ok[1][2])                    # a zero height in slot 1
    st, msg, _, _ = _raw_predict_images(m, bad)
    assert st == SHAPE and "image 1" in msg, (st, msg)
    still_correct()
    bad = list(ok[:4]); bad[3] = (ok[3][0], 10, 32768)                      # a width above 32767 in slot 3
    st, msg, _, _ = _raw_predict_images(m, bad)
    assert st == SHAPE and "image 3" in msg, (st, msg)
    bad = list(ok[:4]); bad[2] = (None, ok[2][1], ok[2][2])                 # a null rgb in slot 2
    st, msg, _, _ = _raw_predict_images(m, bad)
    assert st == INVALID and "image 2" in msg, (st, msg)
    still_correct()
    st, msg, _, _ = _raw_predict_images(m, ok[:4], null_table=True)
    assert st == INVALID, (st, msg)
    still_correct()
    with pytest.raises(_lib().MrcnnError) as e:                             # the Python entry raises the same
        m.predict_images(images)
    assert e.value.code == SHAPE


# ---- paste_masks_source ---------------------------------------------------------------------------------------------------
PASTE_SIZES = [(37, 427), (250, 333), (3, 641), (480, 640), (7, 1)]         # h*w % 4: 3, 2, 3, 0, 3
MODEL_H, MODEL_W = 256, 320


def _synthetic(rows=24, seed=21):
    """Detections in the LETTERBOXED frame of a 256x320 model and 28x28 masks, per image: random boxes as in
    test_gpu_layers.py::test_paste_masks plus the edge cases."""
    E = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
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
        # a box that lies partly in the letterbox border (from above / left of the content into it)
        det[b, 7] = [max(0.0, (py - 9) / (MODEL_H - 1)), max(0.0, (px - 9) / (MODEL_W - 1)), (py + nh * 0.6) / (MODEL_H - 1), (px + nw * 0.6) / (MODEL_W - 1), 7, 0.8]
        det[b, 8] = [0.2, 0.2, 0.6, 0.6, 9, 0.0]                            # score 0: empty mask, box still mapped
    return det, masks


def _expected(det, masks, orc, thr):
    L = _lib().lib()
    det_src = det.copy()
    planes = []
    for b, (h, w) in enumerate(PASTE_SIZES):
        _lib().check(L.mrcnn_unletterbox_boxes(det_src[b].ctypes.data, det.shape[1], 6, h, w, MODEL_H, MODEL_W))
        planes.append(orc.paste_masks(det_src[b], masks[b], h, w, thr))
    return det_src, planes


def test_paste_masks_source_any_width(pkg, orc):
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    det, masks = _synthetic()
    assert any((h * w) % 4 for h, w in PASTE_SIZES)
    want_src, want = _expected(det, masks, orc, 0.5)
    det_src, planes = D.paste_masks_source(det, masks, PASTE_SIZES, MODEL_H, MODEL_W, 0.5)
    np.testing.assert_array_equal(det_src, want_src)
    for b, (h, w) in enumerate(PASTE_SIZES):
        assert planes[b].shape == (det.shape[1], h, w) and planes[b].dtype == np.uint8
        np.testing.assert_array_equal(planes[b], want[b], err_msg=f"image {b} {h}x{w}")
        assert set(np.unique(planes[b])) <= {0, 1}
        assert planes[b][5].sum() == 0 and not det_src[b, 5].any()          # the padding row
        assert planes[b][8].sum() == 0                                      # score 0
        assert planes[b][3].all() == (masks[b, 3] >= 0.5).all()
        if w % 4 == 0:                                                      # the existing entry agrees where it applies
            np.testing.assert_array_equal(planes[b], D.paste_masks(det_src[b], masks[b], h, w, 0.5))
    assert sum(int(p.sum()) for p in planes) > 0


@pytest.mark.parametrize("shift", [0, 5])
def test_paste_masks_source_on_the_device_leaves_the_gaps_alone(pkg, orc, shift):
    """Device buffers, offsets with gaps between the images' planes, the buffer filled with 0xAA first: every byte no plane covers
    is untouched.  shift = 5: `out` itself is not 16-byte aligned (the kernel aligns its wide stores to the ADDRESS)."""
    import torch
    lib = _lib()
    det, masks = _synthetic(rows=12, seed=22)
    rows = det.shape[1]
    want_src, want = _expected(det, masks, orc, 0.5)
    nbytes = [rows * h * w for h, w in PASTE_SIZES]
    offs, pos = [], 48                                                      # a gap in front, a ragged gap after every image
    for n in nbytes:
        offs.append(pos)
        pos = (pos + n + 15) // 16 * 16 + 32
    total = pos
    buf = torch.full((total + shift + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    out = buf[shift:]
    det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    src_g = torch.full(det.shape, -1.0, dtype=torch.float32, device="cuda")
    hs = np.array([s[0] for s in PASTE_SIZES], np.int32); ws = np.array([s[1] for s in PASTE_SIZES], np.int32)
    offs_a = np.array(offs, np.int64)
    lib.check(lib.lib().mrcnn_paste_masks_source(det_g.data_ptr(), masks_g.data_ptr(), len(PASTE_SIZES), rows, 28, hs.ctypes.data, ws.ctypes.data,
                                                 MODEL_H, MODEL_W, C.c_float(0.5), lib.DEVICE, src_g.data_ptr(), out.data_ptr(), offs_a.ctypes.data))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(src_g.cpu().numpy(), want_src)
    covered = np.zeros(got.size, bool)
    for b, (h, w) in enumerate(PASTE_SIZES):
        lo = shift + offs[b]
        np.testing.assert_array_equal(got[lo:lo + nbytes[b]].reshape(rows, h, w), want[b], err_msg=f"image {b} {h}x{w}")
        covered[lo:lo + nbytes[b]] = True
    assert (got[~covered] == 0xAA).all(), f"{int((got[~covered] != 0xAA).sum())} bytes outside the described planes were written"


def test_paste_masks_source_refuses_bad_arguments(pkg):
    lib = _lib()
    det, masks = _synthetic(rows=12)
    rows = det.shape[1]
    hs = np.array([s[0] for s in PASTE_SIZES], np.int32); ws = np.array([s[1] for s in PASTE_SIZES], np.int32)
    out = np.zeros(1 << 23, np.uint8)
    src = np.zeros_like(det)

    def call(hs, ws, offs):
        offs = np.array(offs, np.int64)
        st = lib.lib().mrcnn_paste_masks_source(det.ctypes.data, masks.ctypes.data, len(PASTE_SIZES), rows, 28, hs.ctypes.data, ws.ctypes.data, MODEL_H, MODEL_W,
                                                C.c_float(0.5), lib.HOST, src.ctypes.data, out.ctypes.data, offs.ctypes.data)
        return st, lib.lib().mrcnn_last_error().decode(errors="replace")
    good = [0, 1 << 20, 2 << 20, 3 << 20, 7 << 20]                         # (the largest image's planes: 12 x 480 x 640 = 3.7 MB)
    assert call(hs, ws, good)[0] == 0
    st, msg = call(hs, ws, [0, (1 << 20) + 4, 2 << 20, 3 << 20, 7 << 20])   # not a multiple of 16
    assert st == 1 and "image 1" in msg, (st, msg)
    st, msg = call(hs, ws, [0, 16, 2 << 20, 3 << 20, 7 << 20])              # image 1's planes inside image 0's
    assert st == 1 and "overlap" in msg, (st, msg)
    bad_h = hs.copy(); bad_h[2] = 0
    st, msg = call(bad_h, ws, good)
    assert st == 4 and "image 2" in msg, (st, msg)


def test_evaluate_batched_gives_the_same_results_proto(pkg, small_model):
    E = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
    d, cfg = small_model
    m = _models().load_maskrcnn(d, max_batch=4)
    sizes = [(96, 160), (300, 200), (128, 128), (37, 53), (64, 427), (333, 100), (200, 201)]
    items = [(50 - i, im) for i, im in enumerate(_mixed(sizes, seed=11))]
    blob1, secs1, recs1 = E.evaluate(m, items, limit=None, verbose=False, batch=1)
    blob4, secs4, recs4 = E.evaluate(m, items, limit=None, verbose=False, batch=4)
    assert blob4 == blob1
    assert len(secs4) == 7 and secs4[0] == secs4[3] and secs4[4] == secs4[6]
    assert sum(len(r.detections) for r in recs1) > 0, "no detection above 0.7: the comparison has no teeth"
    blob3, _, _ = E.evaluate(m, items, limit=5, verbose=False, batch=3)
    assert blob3 == E.evaluate(m, items, limit=5, verbose=False)[0]
