"""Drawing run-length masks on the GPU (mrcnn_rle_decode, mrcnn_instance_map_rle, mrcnn_render_detections_rle; detection.rle_decode_planes,
instance_map_rle, render_detections_rle; MaskRCNN.render_tiled, render_tiled_jpegs, instance_pngs_tiled).  Every comparison is byte for
byte: the device entries against their sequential host definitions (pinned against the numpy restatement in tests/test_rle_draw_host.py),
from host memory and from device tensors; the new kernels against the 28x28-mask kernels on the same planes and boxes; the bytes between
the images of a ragged output; a bad RLE in a device-resident set; and the tiled renderers end to end.

The kernel's tile is 32 rows x 256 columns and its cull list holds 256 RLEs (kernels_rle_draw.hip): the shapes below sit on both sides of
each."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tiles_cases as TC
import unite_cases as UC
from test_gpu_render import _sources, _synthetic
from test_render_host import pixel_boxes, restate

pytestmark = pytest.mark.gpu

TH, TW, LIST = 32, 256, 256
RENDER_CASES = [(128, 3), (256, 1), (0, 0)]                                  # (alpha, stroke)
SHAPE = 4


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- the cases: (det_src (B, slots, 6), rles, sizes) --------------------------------------------------------------------------
def _blobs(rng, h, w, n, fill=0.5):
    """n random planes of an h x w image: a rectangle of noise each (density `fill`), and the row that goes with it (its tight box)."""
    CR = _cr()
    det, rles = np.zeros((n, 6), np.float32), []
    for i in range(n):
        y1, x1 = int(rng.integers(0, h)), int(rng.integers(0, w))
        y2, x2 = int(rng.integers(y1, h)) + 1, int(rng.integers(x1, w)) + 1
        plane = np.zeros((h, w), np.uint8)
        plane[y1:y2, x1:x2] = rng.random((y2 - y1, x2 - x1)) < fill
        rles.append(CR.rle_encode(plane))
        det[i] = [y1 / max(1, h - 1), x1 / max(1, w - 1), (y2 - 1) / max(1, h - 1), (x2 - 1) / max(1, w - 1), 1 + i % 7, 0.95 - 0.9 * i / max(1, n)]
    return det, rles


def _batch(seed, sizes, slots, fill=0.5):
    rng = np.random.default_rng(seed)
    parts = [_blobs(rng, h, w, slots, fill) for h, w in sizes]
    return np.stack([p[0] for p in parts]), [p[1] for p in parts], list(sizes)


def _many_slots():
    """300 slots in one image: more than one cull pass.  Rows 3 and 200 are drawn and large, most of the others have a score of 0 (their
    planes are set all the same), the last twenty are drawn: owners found in the first pass must survive the second."""
    det, rles, sizes = _batch(7, [(40, 70)], 300, fill=0.7)
    keep = np.zeros(300, bool)
    keep[[3, 200]] = True
    keep[280:] = True
    det[0, ~keep, 5] = 0
    return det, rles, sizes


def _checkerboard():
    """96 x 96, one-pixel checkerboard: 9216 runs in slot 0 (more than any LDS staging of a run table would hold), a blob below it."""
    det, rles, sizes = _batch(9, [(96, 96)], 2)
    rles[0][0] = {"size": [96, 96], "counts": np.ones(96 * 96, np.uint32)}
    det[0, 0] = [0, 0, 1, 1, 3, 0.9]
    return det, rles, sizes


_CASES = {}


def cases():
    if not _CASES:
        D = _det()
        for sc in UC.scenes():
            args = (sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5)
            for tag, res in (("merge", D.merge_tiles_host(*args, "ios", 0.5, sc["max_out"])), ("unite", D.unite_tiles_host(*args, "iou", 0.5, sc["max_out"]))):
                _CASES[f"{sc['name']}/{tag}"] = (res[0], res[3], [tuple(s) for s in sc["sizes"]])
        _CASES["ragged"] = _batch(1, [(37, 53), (64, 200), (1, 1)], 5)
        _CASES["tile_sides"] = _batch(2, [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1)], 4)
        _CASES["many_slots"] = _many_slots()
        _CASES["checkerboard"] = _checkerboard()
    return _CASES


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _min_scores(det_src):
    s = np.unique(det_src[..., 5][det_src[..., 5] > 0])
    return [0.0, float(s[len(s) // 2]) if len(s) else 0.5]


# ---- 1. device equals host definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scenes", "ragged", "tile_sides", "many_slots", "checkerboard"])
def test_the_device_entries_equal_their_host_definitions(pkg, name):
    D = _det()
    picked = {k: v for k, v in cases().items() if (k == name or (name == "scenes" and "/" in k))}
    assert picked
    for n, (tag, (det_src, rles, sizes)) in enumerate(picked.items()):
        det_g = _cuda(det_src)
        # decode
        want = D.rle_decode_planes_host(rles, sizes)
        got = D.rle_decode_planes(rles, sizes)
        got_g = D.rle_decode_planes(rles, sizes, device="cuda")
        for b in range(len(sizes)):
            np.testing.assert_array_equal(got[b], want[b], err_msg=f"{tag} decode host memspace image {b}")
            np.testing.assert_array_equal(got_g[b].cpu().numpy(), want[b], err_msg=f"{tag} decode device memspace image {b}")
        # map
        for min_score in _min_scores(det_src):
            w_maps, w_vis = D.instance_map_rle_host(det_src, rles, sizes, min_score)
            maps, vis = D.instance_map_rle(det_src, rles, sizes, min_score)
            maps_g, vis_g = D.instance_map_rle(det_g, rles, sizes, min_score)
            np.testing.assert_array_equal(vis, w_vis, err_msg=f"{tag} visible host memspace")
            np.testing.assert_array_equal(vis_g.cpu().numpy().view(np.uint32), w_vis, err_msg=f"{tag} visible device memspace")
            for b in range(len(sizes)):
                np.testing.assert_array_equal(maps[b], w_maps[b], err_msg=f"{tag} map host memspace image {b}")
                np.testing.assert_array_equal(maps_g[b].cpu().numpy(), w_maps[b], err_msg=f"{tag} map device memspace image {b}")
        # render
        images = _images(sizes, 50 + n)
        images_g = [_cuda(im) for im in images]
        for alpha, stroke in RENDER_CASES:
            min_score = _min_scores(det_src)[(alpha // 128) % 2]
            want = D.render_detections_rle_host(images, det_src, rles, min_score, alpha, stroke)
            got = D.render_detections_rle(images, det_src, rles, min_score, alpha, stroke)
            got_g = D.render_detections_rle(images_g, det_g, rles, min_score, alpha, stroke)
            for b in range(len(sizes)):
                np.testing.assert_array_equal(got[b], want[b], err_msg=f"{tag} render {alpha}/{stroke} host memspace image {b}")
                np.testing.assert_array_equal(got_g[b].cpu().numpy(), want[b], err_msg=f"{tag} render {alpha}/{stroke} device memspace image {b}")


def test_a_pair_of_device_tensors_is_used_in_place(pkg):
    """The (counts, run_offsets) form, as coco_eval.DeviceDetections holds it: CUDA tensors in, tensors out, the same bytes."""
    import torch
    D = _det()
    det_src, rles, sizes = cases()["ragged"]
    counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
    offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
    pair = (_cuda(counts.view(np.int32)), _cuda(offs))
    planes = D.rle_decode_planes(pair, sizes)
    maps, vis = D.instance_map_rle(_cuda(det_src), pair, sizes)
    w_planes, (w_maps, w_vis) = D.rle_decode_planes_host(rles, sizes), D.instance_map_rle_host(det_src, rles, sizes)
    assert all(torch.is_tensor(p) and p.is_cuda for p in planes + maps) and vis.is_cuda
    for b in range(len(sizes)):
        np.testing.assert_array_equal(planes[b].cpu().numpy(), w_planes[b])
        np.testing.assert_array_equal(maps[b].cpu().numpy(), w_maps[b])
    np.testing.assert_array_equal(vis.cpu().numpy().view(np.uint32), w_vis)


# ---- 2. the new kernels against the old ones -------------------------------------------------------------------------------------
OLD_SIZES = [(37, 427), (250, 333), (2, 5), (7, 1), (96, 150)]
MODEL_H, MODEL_W = 256, 320


def test_the_rle_kernels_equal_the_mask_kernels(pkg):
    """masks_rle_source's RLEs are the planes instance_map_source and render_detections_source decide their pixels with, and its
    det_src rows denormalise to their boxes: the two families must draw the same bytes."""
    D = _det()
    det, masks = _synthetic(OLD_SIZES)
    images = _sources(OLD_SIZES)
    det_src, rles, _areas, _bboxes = D.masks_rle_source(det, masks, OLD_SIZES, MODEL_H, MODEL_W, 0.5)
    for min_score in (0.0, 0.7):
        _, w_maps, w_vis = D.instance_map_source(det, masks, OLD_SIZES, MODEL_H, MODEL_W, 0.5, min_score)
        maps, vis = D.instance_map_rle(det_src, rles, OLD_SIZES, min_score)
        np.testing.assert_array_equal(vis, w_vis)
        assert int(w_vis.sum()) > 0
        for b in range(len(OLD_SIZES)):
            np.testing.assert_array_equal(maps[b], w_maps[b], err_msg=f"image {b} min_score {min_score}")
    for alpha, stroke in [(128, 3), (256, 3), (0, 0), (77, 1), (128, 8)]:
        want = D.render_detections_source(images, det, masks, MODEL_H, MODEL_W, 0.5, 0.7, alpha, stroke)
        got = D.render_detections_rle(images, det_src, rles, 0.7, alpha, stroke)
        for b in range(len(OLD_SIZES)):
            np.testing.assert_array_equal(got[b], want[b], err_msg=f"image {b} alpha {alpha} stroke {stroke}")


# ---- 3. and 4. the raw entries on device buffers: gaps, a bad RLE ---------------------------------------------------------------------
def _flat(rles):
    counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
    offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
    return counts, offs


def _raw(entry, det_src, counts, offs, sizes, slots, out_offs, total, images=None, fill=0x5a):
    """One call of a device entry with MRCNN_DEVICE on torch buffers; the output buffer (`total` bytes) is pre-filled.  Returns
    (status, message, out bytes as numpy, visible as numpy)."""
    import torch
    lib = _lib()
    L = lib.lib()
    B = len(sizes)
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    c_g, o_g, d_g = _cuda(counts.view(np.int32)), _cuda(offs), _cuda(det_src)
    out = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
    vis = torch.full((B * slots,), 77, dtype=torch.int32, device="cuda")
    out_offs = np.asarray(out_offs, np.int64)
    if entry == "decode":
        st = L.mrcnn_rle_decode(c_g.data_ptr(), o_g.data_ptr(), B, slots, hs.ctypes.data, ws.ctypes.data, lib.DEVICE, out.data_ptr(), out_offs.ctypes.data)
    elif entry == "map":
        st = L.mrcnn_instance_map_rle(d_g.data_ptr(), c_g.data_ptr(), o_g.data_ptr(), B, slots, hs.ctypes.data, ws.ctypes.data, C.c_float(0.0), lib.DEVICE,
                                      out.data_ptr(), out_offs.ctypes.data, vis.data_ptr())
    else:
        keep = [_cuda(im) for im in images]
        table = (lib.Image * B)()
        for b, im in enumerate(keep):
            table[b].rgb, table[b].height, table[b].width = im.data_ptr(), int(im.shape[0]), int(im.shape[1])
        st = L.mrcnn_render_detections_rle(table, d_g.data_ptr(), c_g.data_ptr(), o_g.data_ptr(), B, slots, C.c_float(0.0), 128, 3, lib.DEVICE, out.data_ptr(),
                                           out_offs.ctypes.data)
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), out.cpu().numpy(), vis.cpu().numpy()


def _host_bytes(entry, det_src, rles, sizes, images):
    """The host definition's bytes per image, flat."""
    D = _det()
    if entry == "decode":
        return [p.reshape(-1) for p in D.rle_decode_planes_host(rles, sizes)]
    if entry == "map":
        return [m.reshape(-1).view(np.uint8) for m in D.instance_map_rle_host(det_src, rles, sizes, 0.0)[0]]
    return [r.reshape(-1) for r in D.render_detections_rle_host(images, det_src, rles, 0.0, 128, 3)]


@pytest.mark.parametrize("entry", ["decode", "map", "render"])
def test_the_bytes_between_the_images_stay(pkg, entry):
    det_src, rles, sizes = cases()["ragged"]
    slots = det_src.shape[1]
    images = _images(sizes, 3)
    counts, offs = _flat(rles)
    want = _host_bytes(entry, det_src, rles, sizes, images)
    for shift in (16, 48):
        out_offs, at = [], shift
        for w in want:                                                      # a gap of `shift` bytes (or up to 15 more) before every image
            out_offs.append(at)
            at = (at + len(w) + 15) // 16 * 16 + shift
        st, msg, out, _vis = _raw(entry, det_src, counts, offs, sizes, slots, out_offs, at, images)
        assert st == 0, msg
        covered = np.zeros(at, bool)
        for o, w in zip(out_offs, want):
            np.testing.assert_array_equal(out[o:o + len(w)], w, err_msg=f"{entry} shift {shift}")
            covered[o:o + len(w)] = True
        assert (out[~covered] == 0x5a).all(), f"{entry} shift {shift}: bytes outside the images were written"


@pytest.mark.parametrize("entry", ["decode", "map", "render"])
def test_a_bad_rle_on_the_device_is_named_and_nothing_is_written(pkg, entry):
    det_src, rles, sizes = cases()["ragged"]
    slots = det_src.shape[1]
    images = _images(sizes, 3)
    counts, offs = _flat(rles)
    k = slots + 2                                                           # image 1, slot 2
    padded = [(len(w) + 15) // 16 * 16 for w in _host_bytes(entry, det_src, rles, sizes, images)]
    total, out_offs = sum(padded), np.concatenate(([0], np.cumsum(padded)[:-1]))
    for delta in (1, -1):
        bad = counts.copy()
        j = offs[k] + (0 if delta > 0 else int(np.flatnonzero(counts[offs[k]:offs[k + 1]])[0]))
        bad[j] = np.uint32(int(bad[j]) + delta)                                 # (-1 on a run that has a pixel to give)
        st, msg, out, vis = _raw(entry, det_src, bad, offs, sizes, slots, out_offs, total, images)
        assert st == SHAPE and f"RLE {k} " in msg and str(64 * 200 + delta) in msg, msg
        assert (out == 0x5a).all() and (vis == 77).all()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
E2E_SIZES = [(200, 333), (300, 260)]


@pytest.fixture(scope="module")
def tiled(pkg, small_model):
    d, cfg = small_model
    m = importlib.import_module("mask-rcnn-coreml_amd.models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    return m, [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in E2E_SIZES]


@pytest.mark.parametrize("unite", [True, False])
def test_the_tiled_renderers_draw_what_predict_tiled_returns(tiled, unite):
    import torch
    CR = _cr()
    png = importlib.import_module("mask-rcnn-coreml_amd.png")
    jpeg = importlib.import_module("mask-rcnn-coreml_amd.jpeg")
    m, images = tiled
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=unite, link_threshold=0.25, match_threshold=0.5)
    det_src, source, _n, rles = m.predict_tiled(images, **kw)
    assert (source >= 0).any()
    planes = [np.stack([CR.rle_decode(r) for r in row]) for row in rles]
    got = m.render_tiled(images, min_score=0.0, alpha=128, stroke=3, **kw)
    got_g = m.render_tiled([_cuda(im) for im in images], min_score=0.0, alpha=128, stroke=3, **kw)
    files = m.instance_pngs_tiled(images, min_score=0.0, **kw)
    for b, (h, w) in enumerate(E2E_SIZES):
        inst, _vis, _ring, rgb = restate(pixel_boxes(det_src[b], h, w), det_src[b, :, 5], planes[b], 0.0, 3, 128, images[b])
        assert (inst >= 0).any()
        np.testing.assert_array_equal(got[b], rgb)
        assert torch.is_tensor(got_g[b]) and got_g[b].is_cuda
        np.testing.assert_array_equal(got_g[b].cpu().numpy(), rgb)
        p = png.parse(files[b])
        assert p["palette"] is not None
        np.testing.assert_array_equal(p["scanlines"].astype(np.int64), inst.astype(np.int64) + 1)
    jpegs = m.render_tiled_jpegs(images, min_score=0.0, **kw)
    for b, (h, w) in enumerate(E2E_SIZES):
        assert jpeg.decode_host(jpegs[b]).shape == (h, w, 3)


def test_instance_pngs_tiled_names_max_out(tiled):
    m, images = tiled
    with pytest.raises(ValueError, match="max_out"):
        m.instance_pngs_tiled(images, max_out=256)
