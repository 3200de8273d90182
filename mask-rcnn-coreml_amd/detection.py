"""Result decoding: the public ``Detection`` type and ``IOU`` of the reference library target
(``Sources/Mask-RCNN-CoreML/Detection.swift:15-99``, ``Utils.swift:232``), plus the mask
paste that the example app performs when drawing (``Example/Source/DetectionRenderer.swift:13-24``).
Host-side like the reference; the arithmetic lives in libmaskrcnn_hip.so (``mrcnn_detections_decode``,
``mrcnn_mask_to_u8``, ``mrcnn_iou``).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _lib, _marshal
from ._marshal import Space, image_table, ragged_output, rle_results, sizes_of


@dataclass
class Detection:
    index: int
    boundingBox: Tuple[float, float, float, float]   # CGRect(x, y, width, height), normalized
    classId: int
    score: float
    mask: Optional[np.ndarray]                       # 28×28 uint8 (the CGImage mask's bytes) or None

    @staticmethod
    def detectionsFromFeatureValue(featureValue: np.ndarray, maskFeatureValue: Optional[np.ndarray] = None) -> List["Detection"]:
        """featureValue: "detections" (N,6) float32; maskFeatureValue: "mask" (N,28,28) float32."""
        det = np.ascontiguousarray(featureValue, dtype=np.float32)
        if det.ndim != 2 or det.shape[1] < 6:
            return []
        n = det.shape[0]
        recs = (_lib.DetectionRecord * max(1, n))()
        cnt = C.c_int64(0)
        _lib.check(_lib.lib().mrcnn_detections_decode(det.ctypes.data, n, det.shape[1], recs, n, C.byref(cnt)))
        out = []
        for k in range(cnt.value):
            r = recs[k]
            mask = None
            if maskFeatureValue is not None and maskFeatureValue.shape[0] > r.index:
                mask = Detection.maskFromFeatureValue(maskFeatureValue, r.index)
            out.append(Detection(int(r.index), (r.x, r.y, r.w, r.h), int(r.class_id), float(r.score), mask))
        return out

    @staticmethod
    def maskFromFeatureValue(maskFeatureValue: np.ndarray, atIndex: int) -> Optional[np.ndarray]:
        if maskFeatureValue.shape[0] <= atIndex:
            return None
        m = np.ascontiguousarray(maskFeatureValue[atIndex], dtype=np.float32)
        out = np.empty(m.shape, dtype=np.uint8)
        _lib.check(_lib.lib().mrcnn_mask_to_u8(m.ctypes.data, m.size, out.ctypes.data))
        return out


def IOU(a_xywh, b_xywh) -> float:
    """``IOU(_ a: CGRect, _ b: CGRect) -> Float`` with rects as (x, y, width, height)."""
    def yxyx(r):
        x, y, w, h = r
        return np.array([y, x, y + h, x + w], dtype=np.float32)
    a, b = yxyx(a_xywh), yxyx(b_xywh)
    f32p = C.POINTER(C.c_float)
    return float(_lib.lib().mrcnn_iou(a.ctypes.data_as(f32p), b.ctypes.data_as(f32p)))


def paste_masks(detections: np.ndarray, masks: np.ndarray, image_h: int, image_w: int, threshold: float = 0.5) -> np.ndarray:
    """Full-resolution binary instance masks (n, image_h, image_w) uint8 from "detections" (n,6) and
    "mask" (n,S,S): each mask is resized to its box and thresholded on the GPU (``mrcnn_paste_masks``) —
    the step DetectionRenderer.renderMask (Example/Source/DetectionRenderer.swift:13-24) leaves to
    CoreGraphics when drawing, and the one mask AP needs."""
    det = np.ascontiguousarray(detections, dtype=np.float32)
    m = np.ascontiguousarray(masks, dtype=np.float32)
    n = det.shape[0]
    out = np.empty((n, image_h, image_w), dtype=np.uint8)
    _lib.check(_lib.lib().mrcnn_paste_masks(det.ctypes.data, det.shape[1], m.ctypes.data, n, m.shape[1], image_h, image_w,
                                            C.c_float(threshold), _lib.HOST, out.ctypes.data))
    return out


def paste_masks_source(detections: np.ndarray, masks: np.ndarray, sizes, model_h: int, model_w: int, threshold: float = 0.5):
    """The way back from ``MaskRCNN.predict_images``: detections (B,rows,6) / masks (B,rows,S,S) of a batch of images of sizes
    ``sizes`` = [(h_b, w_b)] → (det_src, [ (rows, h_b, w_b) uint8 per image ]).  det_src holds the boxes normalized in each SOURCE
    image (``mrcnn_unletterbox_boxes``' mapping, done on the GPU), the masks are pasted in each image's own pixels — any width —
    by one launch over the ragged buffer (``mrcnn_paste_masks_source``)."""
    space = Space()
    det, m = space.f32(detections, masks)
    B, rows = det.shape[0], det.shape[1]
    if len(sizes) != B or m.shape[0] != B or m.shape[1] != rows or det.shape[2] != 6:
        raise ValueError("paste_masks_source: detections (B,rows,6), masks (B,rows,S,S) and B sizes expected")
    hs, ws = sizes_of(sizes)
    out, offs, planes = ragged_output(space, hs, ws, np.uint8, lead=(rows,))
    det_src = np.empty_like(det)
    _lib.check(_lib.lib().mrcnn_paste_masks_source(det.ctypes.data, m.ctypes.data, B, rows, m.shape[2], hs.ctypes.data, ws.ctypes.data,
                                                   model_h, model_w, C.c_float(threshold), _lib.HOST, det_src.ctypes.data,
                                                   out.ctypes.data, offs.ctypes.data))
    return det_src, planes()


def masks_rle_source(detections, masks, sizes, model_h: int, model_w: int, threshold: float = 0.5):
    """The masks ``paste_masks_source`` would paste, as COCO run-length encodings straight from the GPU — the planes never exist
    (``mrcnn_masks_rle_source``).  Same arguments; returns (det_src, rles, areas, bboxes): ``rles[b][i] = {"size": [h_b, w_b],
    "counts": uint32 array}`` (column-major runs, coco_results.rle_decode gives the plane back), areas (B, rows) the set pixels,
    bboxes (B, rows, 4) their tight box x, y, w, h.  numpy in → numpy out.  torch CUDA tensors in → the device buffers are used in
    place, det_src / areas / bboxes stay on the device (int32 tensors) and only the run offsets and the used part of the run
    lengths come to the host.  A first attempt is sized from the image widths; if the batch needs more, one more call with the
    capacity the library reported."""
    space = Space(detections)
    ptr = space.ptr
    det, m = space.f32(detections, masks)
    B, rows = int(det.shape[0]), int(det.shape[1])
    if len(sizes) != B or m.shape[0] != B or m.shape[1] != rows or det.shape[2] != 6:
        raise ValueError("masks_rle_source: detections (B,rows,6), masks (B,rows,S,S) and B sizes expected")
    hs, ws = sizes_of(sizes)
    det_src, areas, bboxes = space.new(det.shape, np.float32), space.new((B, rows), np.uint32), space.new((B, rows, 4), np.int32)

    def call(counts, capacity, run_offsets):
        return _lib.lib().mrcnn_masks_rle_source(ptr(det), ptr(m), B, rows, int(m.shape[2]), hs.ctypes.data, ws.ctypes.data, model_h, model_w,
                                                 C.c_float(threshold), space.code, ptr(det_src), ptr(counts), capacity, ptr(run_offsets),
                                                 ptr(areas), ptr(bboxes))
    # a mask with one run of ones per column of its image has 2 w + 1 runs: enough for the masks a network draws, not for noise
    rles = rle_results(space, B, rows, hs, ws, int(rows * (2 * ws.astype(np.int64) + 2).sum()), call)
    return det_src, rles, areas, bboxes


def tile_plan(height: int, width: int, tile, overlap=(64, 64), image: int = 0) -> np.ndarray:
    """The windows of one image (``mrcnn_tile_plan``): tile = (tile_h, tile_w), overlap = (overlap_y, overlap_x) → an (n, 5) int32
    array of (image, y0, x0, height, width), row-major.  Per axis: one window if the image is not longer than the tile, else windows
    of exactly the tile's length at stride tile - overlap, the last one shifted inward.  The tables of several images are
    concatenated with np.concatenate."""
    n = C.c_int(0)
    args = (int(height), int(width), int(tile[0]), int(tile[1]), int(overlap[0]), int(overlap[1]), int(image))
    _lib.check(_lib.lib().mrcnn_tile_plan(*args, None, 0, C.byref(n)))
    out = np.zeros((n.value, 5), dtype=np.int32)
    _lib.check(_lib.lib().mrcnn_tile_plan(*args, out.ctypes.data_as(C.POINTER(_lib.Tile)), n.value, C.byref(n)))
    return out


def _tile_table(tiles):
    t = np.ascontiguousarray(tiles, dtype=np.int32)
    if t.ndim != 2 or t.shape[1] != 5:
        raise ValueError("tiles: an (n, 5) table of (image, y0, x0, height, width) expected")
    return t


_METRICS = {"iou": _lib.MATCH_IOU, "ios": _lib.MATCH_IOS}


def _merge_tiles(host_definition, detections, masks, tiles, sizes, model_h, model_w, threshold, metric, match_threshold, max_out, unite=False,
                 resident=None):
    name = "unite_tiles" if unite else "merge_tiles"
    space = Space(detections)
    ptr = space.ptr
    assert space.on_host or not host_definition, f"{name}_host takes numpy arrays"
    det, m = space.f32(detections, masks)
    tab = _tile_table(tiles)
    T, rows = int(det.shape[0]), int(det.shape[1])
    if tab.shape[0] != T or m.shape[0] != T or m.shape[1] != rows or det.shape[2] != 6:
        raise ValueError(f"{name}: detections (T,rows,6), masks (T,rows,S,S) and T tiles expected")
    if metric not in _METRICS:
        raise ValueError(f"{name}: metric {metric!r} is neither 'iou' nor 'ios'")
    B = len(sizes)
    hs, ws = sizes_of(sizes)
    max_out = int(rows if max_out is None else max_out)
    per = max(0, max_out)
    z = lambda shape, dt: space.new(shape, dt, zero=True)
    det_src, source, n_kept = z((B, per, 6), np.float32), z((B, per), np.int32), z((B,), np.int32)
    areas, bboxes = z((B, per), np.uint32), z((B, per, 4), np.int32)
    n_parts, group = z((B, per), np.int32), z((T, rows), np.int32)
    head = (ptr(det), ptr(m), tab.ctypes.data_as(C.POINTER(_lib.Tile)), T, rows, int(m.shape[2]), hs.ctypes.data, ws.ctypes.data, B,
            int(model_h), int(model_w), C.c_float(threshold), _METRICS[metric], float(match_threshold), max_out)

    def call(counts, capacity, run_offsets):
        parts = (ptr(n_parts), ptr(group)) if unite else ()
        tail = (ptr(det_src), ptr(source), ptr(n_kept), *parts, ptr(counts), capacity, ptr(run_offsets), ptr(areas), ptr(bboxes))
        if host_definition:
            return getattr(_lib.lib(), f"mrcnn_{name}_host")(*head, *tail)
        return getattr(_lib.lib(), f"mrcnn_{name}")(*head, space.code, *tail)
    # the first attempt is sized as masks_rle_source sizes its own
    rles = rle_results(space, B, max_out, hs, ws, int(max(1, max_out) * (2 * ws.astype(np.int64) + 2).sum()), call, resident)
    if unite:
        return det_src, source, n_kept, rles, areas, bboxes, n_parts, group
    return det_src, source, n_kept, rles, areas, bboxes


def merge_tiles(detections, masks, tiles, sizes, model_h: int, model_w: int, threshold: float = 0.5, metric: str = "ios",
                match_threshold: float = 0.5, max_out=None):
    """The records ``MaskRCNN.predict_tiles`` returned for the windows ``tiles`` of images of sizes ``sizes`` = [(h_b, w_b)], in the
    frame of those images, the duplicates of the overlaps dropped on the GPU (``mrcnn_merge_tiles``; the header states the rule).
    Returns (det_src (B, max_out, 6), source (B, max_out) — the candidate tile*rows + row, -1 for padding —, n_kept (B) before the
    cap, rles, areas, bboxes): ``rles[b][j]`` as masks_rle_source returns them, so coco_results.coco_results and
    coco_eval.score_batch take them with det_src as they are.  metric "ios" (intersection over the smaller area: removes the cut
    copy of an object in favour of its whole copy) or "iou"; max_out = None keeps `rows` per image.  numpy in → numpy out; torch
    CUDA tensors in → the outputs stay on the device, only the run lengths come to the host."""
    return _merge_tiles(False, detections, masks, tiles, sizes, model_h, model_w, threshold, metric, match_threshold, max_out)


def merge_tiles_host(detections, masks, tiles, sizes, model_h: int, model_w: int, threshold: float = 0.5, metric: str = "ios",
                     match_threshold: float = 0.5, max_out=None):
    """The definition of merge_tiles: the same arguments (numpy) and results from the sequential host code
    (``mrcnn_merge_tiles_host``), no GPU."""
    return _merge_tiles(True, detections, masks, tiles, sizes, model_h, model_w, threshold, metric, match_threshold, max_out)


def unite_tiles(detections, masks, tiles, sizes, model_h: int, model_w: int, threshold: float = 0.5, metric: str = "iou",
                link_threshold: float = 0.5, max_out=None):
    """merge_tiles' arguments; the cut parts of an object that no window holds whole, and its duplicates, united into one mask on the
    GPU (``mrcnn_unite_tiles``; the header states the rule).  Candidates of different tiles and one class are LINKED if their planes
    agree (metric "iou" or "ios" >= link_threshold) inside the rectangle both windows see; every connected component of the links
    becomes one output: the OR of its members' planes, the row of the hull of their boxes, class and score of its best member.
    Returns (det_src, source — the best member's candidate index —, n_kept — the components before the cap —, rles, areas, bboxes,
    n_parts (B, max_out) — the members per output —, group (T, rows) — per candidate its output's index in its image, -1 if not
    eligible).  ``rles[b][j]`` go to coco_results.coco_results and coco_eval.score_batch with det_src as they are; a united mask is
    no pasted S x S mask any more: rle_decode_planes, instance_map_rle and render_detections_rle draw it from its RLE."""
    return _merge_tiles(False, detections, masks, tiles, sizes, model_h, model_w, threshold, metric, link_threshold, max_out, unite=True)


def unite_tiles_host(detections, masks, tiles, sizes, model_h: int, model_w: int, threshold: float = 0.5, metric: str = "iou",
                     link_threshold: float = 0.5, max_out=None):
    """The definition of unite_tiles: the same arguments (numpy) and results from the sequential host code
    (``mrcnn_unite_tiles_host``), no GPU."""
    return _merge_tiles(True, detections, masks, tiles, sizes, model_h, model_w, threshold, metric, link_threshold, max_out, unite=True)


def _batch_inputs(name, detections, masks, B_expected):
    """(space, det, masks, B, rows): numpy arrays made contiguous float32, or contiguous float32 CUDA tensors used in place."""
    space = Space(detections)
    det, m = space.f32(detections, masks)
    if det.ndim != 3 or m.ndim != 4 or det.shape[2] != 6 or m.shape[0] != det.shape[0] or m.shape[1] != det.shape[1] or B_expected != det.shape[0]:
        raise ValueError(f"{name}: detections (B,rows,6), masks (B,rows,S,S) and B images / sizes expected")
    return space, det, m, int(det.shape[0]), int(det.shape[1])


def instance_map_source(detections, masks, sizes, model_h: int, model_w: int, threshold: float = 0.5, min_score: float = 0.0):
    """Which detection owns a pixel (``mrcnn_instance_map_source``): for a batch of images of sizes ``sizes`` = [(h_b, w_b)] returns
    (det_src, [ (h_b, w_b) int16 per image ], visible (B, rows) uint32).  ``map[y, x]`` is the lowest row with score > min_score whose
    pasted mask (``paste_masks_source`` at ``threshold``) is set at the pixel, -1 where there is none; ``visible[b, i]`` counts the
    pixels row i owns.  The planes are never pasted.  numpy in → numpy out; torch CUDA tensors in → the device buffers are used in
    place and torch tensors come back (visible as int32)."""
    sizes = list(sizes)
    space, det, m, B, rows = _batch_inputs("instance_map_source", detections, masks, len(sizes))
    ptr = space.ptr
    hs, ws = sizes_of(sizes)
    out, offs, maps = ragged_output(space, hs, ws, np.int16)
    det_src, visible = space.new(det.shape, np.float32), space.new((B, rows), np.uint32, zero=True)
    _lib.check(_lib.lib().mrcnn_instance_map_source(ptr(det), ptr(m), B, rows, int(m.shape[2]), hs.ctypes.data, ws.ctypes.data, model_h, model_w,
                                                    C.c_float(threshold), C.c_float(min_score), space.code,
                                                    ptr(det_src), ptr(out), offs.ctypes.data, ptr(visible)))
    return det_src, maps(), visible


def render_detections_source(images, detections, masks, model_h: int, model_w: int, threshold: float = 0.5, min_score: float = 0.7,
                             alpha: int = 128, stroke: int = 3):
    """The detections drawn over their source images (``mrcnn_render_detections_source``; DetectionRenderer.swift:26-88): a list of
    (h_b, w_b, 3) uint8 images and the (det, mask) ``MaskRCNN.predict_images`` returned for them → [ (h_b, w_b, 3) uint8 ].  Rows with
    score > min_score (0.7: the cut Detection.swift:38 applies before drawing) are drawn in palette[i % 4] = red, blue, green, yellow:
    the box stroked ``stroke`` pixels wide, opaque, the mask blended in with ``alpha``/256 (256 = the reference's opaque fill); the
    lowest row wins a contested pixel.  numpy in → numpy out; torch CUDA tensors in → used in place, torch tensors returned."""
    images = list(images)
    space, det, m, B, rows = _batch_inputs("render_detections_source", detections, masks, len(images))
    ptr = space.ptr
    table, _, keep, hs, ws = image_table(images, space)
    out, offs, drawn = ragged_output(space, hs, ws, np.uint8, trail=(3,))
    _lib.check(_lib.lib().mrcnn_render_detections_source(table, ptr(det), ptr(m), B, rows, int(m.shape[2]), model_h, model_w, C.c_float(threshold),
                                                         C.c_float(min_score), int(alpha), int(stroke), space.code,
                                                         None, ptr(out), offs.ctypes.data))
    return drawn()


# ---- drawing run-length masks (mrcnn_rle_decode, mrcnn_instance_map_rle, mrcnn_render_detections_rle) ------------------------------------
def _rle_rows(name, host_definition, det_src, rles, sizes):
    """(set, space, det_src) of a drawing call: the (B, slots, 6) source-frame rows say where it runs, and the RLE set goes there."""
    space = Space(det_src)
    s = _marshal.RleSet(name, rles, sizes, space.device, host_definition, in_place=False)
    assert space.on_host or not host_definition, f"{name}_host takes numpy arrays"
    det, = space.f32(det_src)
    if det.ndim != 3 or det.shape[0] != s.B or det.shape[1] != s.slots or det.shape[2] != 6:
        raise ValueError(f"{name}: det_src {tuple(det.shape)} does not go with {s.B} images of {s.slots} RLEs: ({s.B}, {s.slots}, 6) expected")
    return s, space, det


def _rle_decode_planes(host_definition, rles, sizes, device):
    s = _marshal.RleSet("rle_decode_planes_host" if host_definition else "rle_decode_planes", rles, sizes, device, host_definition)
    space = s.space
    ptr = space.ptr
    out, out_offs, planes = ragged_output(space, s.image_hs, s.image_ws, np.uint8, lead=(s.slots,))
    head = (ptr(s.counts), ptr(s.offs), s.B, s.slots, s.image_hs.ctypes.data, s.image_ws.ctypes.data)
    if host_definition:
        _lib.check(_lib.lib().mrcnn_rle_decode_host(*head, ptr(out), out_offs.ctypes.data))
    else:
        _lib.check(_lib.lib().mrcnn_rle_decode(*head, space.code, ptr(out), out_offs.ctypes.data))
    return planes()


def rle_decode_planes(rles, sizes=None, device=None):
    """The dense planes of an RLE set, decoded on the GPU (``mrcnn_rle_decode``): [ (slots, h_b, w_b) uint8 {0,1} per image ], the
    layout paste_masks_source returns, so png.encode_batch takes them.  ``rles`` as merge_tiles, unite_tiles and masks_rle_source
    return them — rles[b][i] = {"size", "counts"} — or a (counts, run_offsets) pair with ``sizes`` = [(h_b, w_b)]
    (coco_eval.DeviceDetections and COCOGroundTruth.to_device() hold such pairs).  numpy arrays come back, unless ``device`` is given
    or the pair is CUDA tensors (used in place): then the planes stay on the device as tensors."""
    return _rle_decode_planes(False, rles, sizes, device)


def rle_decode_planes_host(rles, sizes=None):
    """The definition of rle_decode_planes: the sequential host code (``mrcnn_rle_decode_host``), no GPU; numpy out."""
    return _rle_decode_planes(True, rles, sizes, None)


def _instance_map_rle(host_definition, det_src, rles, sizes, min_score):
    name = "instance_map_rle_host" if host_definition else "instance_map_rle"
    s, space, det = _rle_rows(name, host_definition, det_src, rles, sizes)
    ptr = space.ptr
    out, map_offs, maps = ragged_output(space, s.image_hs, s.image_ws, np.int16)
    visible = space.new((s.B, s.slots), np.uint32, zero=True)
    head = (ptr(det), ptr(s.counts), ptr(s.offs), s.B, s.slots, s.image_hs.ctypes.data, s.image_ws.ctypes.data, C.c_float(min_score))
    tail = (ptr(out), map_offs.ctypes.data, ptr(visible))
    if host_definition:
        _lib.check(_lib.lib().mrcnn_instance_map_rle_host(*head, *tail))
    else:
        _lib.check(_lib.lib().mrcnn_instance_map_rle(*head, space.code, *tail))
    return maps(), visible


def instance_map_rle(det_src, rles, sizes=None, min_score: float = 0.0):
    """Which RLE owns a pixel (``mrcnn_instance_map_rle``): det_src (B, slots, 6) source-frame rows and the RLE set that goes with them
    (``rles`` as rle_decode_planes takes them — what merge_tiles, unite_tiles or masks_rle_source returned) → ([ (h_b, w_b) int16 per
    image ], visible (B, slots)).  ``map[y, x]`` is the lowest row with score > min_score, score > 0 and a non-empty box whose mask is
    set at the pixel, -1 where there is none; the box only decides whether a row is drawn.  numpy det_src → numpy out; a CUDA tensor →
    the RLEs are uploaded (a pair of CUDA tensors is used in place) and tensors come back (visible as int32)."""
    return _instance_map_rle(False, det_src, rles, sizes, min_score)


def instance_map_rle_host(det_src, rles, sizes=None, min_score: float = 0.0):
    """The definition of instance_map_rle: the sequential host code (``mrcnn_instance_map_rle_host``), no GPU; numpy in and out."""
    return _instance_map_rle(True, det_src, rles, sizes, min_score)


def _render_detections_rle(host_definition, images, det_src, rles, min_score, alpha, stroke):
    name = "render_detections_rle_host" if host_definition else "render_detections_rle"
    images = list(images)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    s, space, det = _rle_rows(name, host_definition, det_src, rles, sizes)
    ptr = space.ptr
    table, _, keep, hs, ws = image_table(images, space)
    out, out_offs, drawn = ragged_output(space, hs, ws, np.uint8, trail=(3,))
    head = (table, ptr(det), ptr(s.counts), ptr(s.offs), s.B, s.slots, C.c_float(min_score), int(alpha), int(stroke))
    if host_definition:
        _lib.check(_lib.lib().mrcnn_render_detections_rle_host(*head, ptr(out), out_offs.ctypes.data))
    else:
        _lib.check(_lib.lib().mrcnn_render_detections_rle(*head, space.code, ptr(out), out_offs.ctypes.data))
    return drawn()


def render_detections_rle(images, det_src, rles, min_score: float = 0.7, alpha: int = 128, stroke: int = 3):
    """Run-length masks drawn over their images (``mrcnn_render_detections_rle``): a list of (h_b, w_b, 3) uint8 images, det_src
    (B, slots, 6) and the RLE set that goes with it → [ (h_b, w_b, 3) uint8 ].  Stroke, blend and palette are
    render_detections_source's, the mask is the RLE's plane — so the result of predict_tiled, united or not, can be looked at.
    numpy in → numpy out; CUDA tensors in (images and det_src; the RLEs are uploaded, or a pair of CUDA tensors used in place) →
    tensors out."""
    return _render_detections_rle(False, images, det_src, rles, min_score, alpha, stroke)


def render_detections_rle_host(images, det_src, rles, min_score: float = 0.7, alpha: int = 128, stroke: int = 3):
    """The definition of render_detections_rle: the sequential host code (``mrcnn_render_detections_rle_host``), no GPU."""
    return _render_detections_rle(True, images, det_src, rles, min_score, alpha, stroke)


# ---- polygons out (mrcnn_rle_to_polygons) -------------------------------------------------------------------------------------------
def _simplify_flat(host_definition, space, ring_offsets, xy, tolerance):
    """mrcnn_polygons_simplify(_host) on ring_offsets (R + 1) and xy (V, 2) of ``space`` -> (ring_offsets, areas2, xy (V', 2), src_index,
    V').  One call: the input's vertex count always suffices as the capacity."""
    R, V = int(ring_offsets.shape[0]) - 1, int(xy.shape[0])
    if R < 0 or (V and tuple(xy.shape) != (V, 2)):
        raise ValueError("simplify_polygons: ring_offsets needs an entry and xy the shape (V, 2)")
    ptr = space.ptr
    src_xy = xy if V else space.new(2, np.int32, zero=True)      # (an empty tensor has no address)
    out_offsets, areas2 = space.new(R + 1, np.int64, zero=True), space.new(max(1, R), np.int64)
    out_xy, src_index = space.new(max(2, 2 * V), np.int32), space.new(max(1, V), np.int64)
    total = C.c_int64(0)
    head = (ptr(ring_offsets), ptr(src_xy), R, C.c_double(float(tolerance))) + (() if host_definition else (space.code,))
    entry = _lib.lib().mrcnn_polygons_simplify_host if host_definition else _lib.lib().mrcnn_polygons_simplify
    _lib.check(entry(*head, ptr(out_offsets), ptr(areas2), ptr(out_xy), ptr(src_index), C.byref(total), V))
    n = total.value
    return out_offsets, areas2[:R], out_xy[:2 * n].reshape(n, 2), src_index[:n], n


def _flat_of_nested(rings, areas):
    """rings[b][i] = the list of the (m, 2) arrays of RLE i of image b, areas beside them -> (the flat dictionary, every ring in order)"""
    every = [np.asarray(r, dtype=np.int32).reshape(-1, 2) for row in rings for rle in row for r in rle]
    per_rle = [len(rle) for row in rings for rle in row]
    return {"rle_rings": np.concatenate(([0], np.cumsum(per_rle))).astype(np.int64),
            "ring_offsets": np.concatenate(([0], np.cumsum([len(r) for r in every]))).astype(np.int64),
            "ring_areas": np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for row in areas for a in row] + [np.zeros(0, np.int64)]),
            "xy": np.concatenate(every + [np.zeros((0, 2), np.int32)])}, every


def _simplify_polygons(host_definition, polygons, tolerance, device, flat):
    nested = not isinstance(polygons, dict)
    if nested:
        rings, areas = polygons[0], polygons[1]
        P, every = _flat_of_nested(rings, areas)
    else:
        P = dict(polygons)
    on_device = hasattr(P["xy"], "is_cuda")
    if device is None and on_device and not host_definition:
        device = P["xy"].device                                  # tensors: simplified where they lie, tensors out
    space = Space(device)
    here = space.take
    offsets, xy = here(P["ring_offsets"], np.int64), here(P["xy"], np.int32)
    out_offsets, areas2, out_xy, src_index, n = _simplify_flat(host_definition, space, offsets, xy, tolerance)
    out = {"rle_rings": here(P.get("rle_rings"), np.int64), "ring_offsets": out_offsets, "ring_areas": here(P.get("ring_areas"), np.int64),
           "areas2": areas2, "xy": out_xy, "src_index": src_index, "n_rings": int(offsets.shape[0]) - 1, "n_vertices": n}
    if flat or not nested:
        return out
    ro, sxy = space.host(out_offsets), space.host(out_xy)
    at = iter(range(len(every)))
    return [[[sxy[ro[r]:ro[r + 1]] for r in (next(at) for _ in rle)] for rle in row] for row in rings], areas


def simplify_polygons(polygons, tolerance, device=None, flat: bool = False):
    """Polygon rings simplified on the GPU by Douglas-Peucker with ``tolerance`` in pixels (``mrcnn_polygons_simplify``; the rule is
    defined in include/maskrcnn_hip.h: exact in integers, a dropped vertex lies within the tolerance of the chord that replaces it,
    topology is not preserved).  ``polygons`` is what rle_to_polygons returned: the flat dictionary (flat=True) — its ring_offsets and
    xy, numpy arrays or CUDA tensors, which are simplified where they lie — or the nested (rings, areas) pair.  The flat form comes
    back flat: rle_rings and ring_areas as they were (the ORIGINAL pixel areas), ring_offsets and xy simplified, and beside them areas2
    (twice the signed area of each simplified ring), src_index (per vertex, its index in the input xy), n_rings, n_vertices.  The nested
    form comes back nested, (rings, areas) with the original areas, unless flat=True.  Rings stay in their order, one for one; a ring
    may come out with two vertices.  The (rings, areas, nesting) triple of rle_to_polygons(..., nest=True) is taken too: its first two
    entries are simplified and returned, the nesting is not touched and still indexes the rings."""
    return _simplify_polygons(False, polygons, tolerance, device, flat)


def simplify_polygons_host(polygons, tolerance, flat: bool = False):
    """The definition of simplify_polygons: the sequential host code (``mrcnn_polygons_simplify_host``), no GPU; numpy out."""
    return _simplify_polygons(True, polygons, tolerance, None, flat)


def _nest_flat(host_definition, space, rle_rings, ring_offsets, xy):
    """mrcnn_polygons_nest(_host) on rle_rings (K + 1), ring_offsets (R + 1) and xy (V, 2) of ``space`` -> the flat nesting: parent,
    depth, rle_polys, poly_rings (n_polys + 1), ring_order, n_polys.  The buffers are sized by R: one call."""
    K, R, V = int(rle_rings.shape[0]) - 1, int(ring_offsets.shape[0]) - 1, int(xy.shape[0])
    if K < 0 or R < 0 or (V and tuple(xy.shape) != (V, 2)):
        raise ValueError("nest_polygons: rle_rings and ring_offsets need an entry each and xy the shape (V, 2)")
    ptr = space.ptr
    src_xy = xy if V else space.new(2, np.int32, zero=True)      # (an empty tensor has no address)
    parent, depth, ring_order = space.new(max(1, R), np.int64), space.new(max(1, R), np.int32), space.new(max(1, R), np.int64)
    rle_polys, poly_rings = space.new(K + 1, np.int64, zero=True), space.new(R + 1, np.int64, zero=True)
    total = C.c_int64(0)
    head = (ptr(rle_rings), K, ptr(ring_offsets), ptr(src_xy), R) + (() if host_definition else (space.code,))
    entry = _lib.lib().mrcnn_polygons_nest_host if host_definition else _lib.lib().mrcnn_polygons_nest
    _lib.check(entry(*head, ptr(parent), ptr(depth), ptr(rle_polys), ptr(poly_rings), ptr(ring_order), C.byref(total)))
    P = total.value
    return {"parent": parent[:R], "depth": depth[:R], "rle_polys": rle_polys, "poly_rings": poly_rings[:P + 1], "ring_order": ring_order[:R], "n_polys": P}


def _nest_nested(N, rle_rings, per_image):
    """The flat nesting as lists: {"nest": nest[b][i] = [[shell, hole, ...], ...], "parent": parent[b][i], "depth": depth[b][i]}, all
    indices LOCAL to rings[b][i] (parent -1: none).  per_image: the number of RLEs of each image."""
    host = lambda a: a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
    parent, depth, rle_polys, poly_rings, order = (host(N[k]) for k in ("parent", "depth", "rle_polys", "poly_rings", "ring_order"))
    rr = host(rle_rings)
    nest, par, dep, k = [], [], [], 0
    for slots in per_image:
        nest.append([]), par.append([]), dep.append([])
        for _ in range(slots):
            r0, r1 = int(rr[k]), int(rr[k + 1])
            nest[-1].append([[int(r) - r0 for r in order[int(poly_rings[p]):int(poly_rings[p + 1])]] for p in range(int(rle_polys[k]), int(rle_polys[k + 1]))])
            p = parent[r0:r1]
            par[-1].append(np.where(p >= 0, p - r0, -1))
            dep[-1].append(depth[r0:r1].copy())
            k += 1
    return {"nest": nest, "parent": par, "depth": dep}


def _nest_polygons(host_definition, polygons, device, flat):
    nested = not isinstance(polygons, dict)
    if nested:
        rings = polygons[0]
        P, _ = _flat_of_nested(rings, [[np.zeros(len(rle), np.int64) for rle in row] for row in rings])      # (areas are not trusted: not needed)
    else:
        P = dict(polygons)
        if P.get("rle_rings") is None:
            raise ValueError("nest_polygons: the flat form needs rle_rings, ring_offsets and xy")
    if device is None and hasattr(P["xy"], "is_cuda") and not host_definition:
        device = P["xy"].device                                  # tensors: nested where they lie, tensors out
    space = Space(device)
    rle_rings = space.take(P["rle_rings"], np.int64)
    N = _nest_flat(host_definition, space, rle_rings, space.take(P["ring_offsets"], np.int64), space.take(P["xy"], np.int32))
    if flat or not nested:
        return N
    return _nest_nested(N, rle_rings, [len(row) for row in rings])


def nest_polygons(polygons, device=None, flat: bool = False):
    """Polygon rings nested on the GPU into outlines and their holes (``mrcnn_polygons_nest``; the rule is defined in
    include/maskrcnn_hip.h: a ring's parent is the closest ring of its RLE that contains the centre of the pixel at the ring's first
    vertex, even depth is a shell, its children are its holes).  ``polygons`` is what rle_to_polygons or simplify_polygons returned:
    the flat dictionary — rle_rings, ring_offsets and xy, numpy arrays or CUDA tensors, which are nested where they lie — or the
    nested (rings, areas) pair.  The flat form (and flat=True) gives the library's arrays: parent (global ring indices, -1: none),
    depth, rle_polys, poly_rings, ring_order — polygon p owns ring_order[poly_rings[p]:poly_rings[p + 1]], shell first, and RLE k the
    polygons rle_polys[k]:rle_polys[k + 1] — and n_polys.  The nested form gives {"nest", "parent", "depth"}: nest[b][i] =
    [[shell_ring, hole_ring, ...], ...], indices into rings[b][i], and parent[b][i], depth[b][i] per ring with local indices too.
    Nest the TRACED rings: simplification keeps rings one for one, so the result indexes the simplified rings, whose own topology is
    not preserved."""
    return _nest_polygons(False, polygons, device, flat)


def nest_polygons_host(polygons, flat: bool = False):
    """The definition of nest_polygons: the sequential host code (``mrcnn_polygons_nest_host``), no GPU; numpy out."""
    return _nest_polygons(True, polygons, None, flat)


def _rle_to_polygons(host_definition, rles, sizes, device, flat, tolerance=None, nest=False):
    name = "rle_to_polygons_host" if host_definition else "rle_to_polygons"
    s = _marshal.RleSet(name, rles, sizes, device, host_definition)
    space, B, slots, n = s.space, s.B, s.slots, s.n
    ptr = space.ptr
    rle_rings = space.new(n + 1, np.int64, zero=True)
    totals = (C.c_int64(0), C.c_int64(0))
    head = (ptr(s.counts), ptr(s.offs), B, slots, s.image_hs.ctypes.data, s.image_ws.ctypes.data) + (() if host_definition else (space.code,))
    entry = getattr(_lib.lib(), "mrcnn_" + name)

    def attempt(capacity):                                       # rings and vertices grow together
        cap_r, cap_v = capacity
        ring_offsets, ring_areas, xy = space.new(cap_r + 1, np.int64), space.new(max(1, cap_r), np.int64), space.new(max(1, 2 * cap_v), np.int32)
        st = entry(*head, ptr(rle_rings), C.byref(totals[0]), C.byref(totals[1]), ptr(ring_offsets), ptr(ring_areas), cap_r, ptr(xy), cap_v)
        return st, (totals[0].value, totals[1].value), (ring_offsets, ring_areas, xy)
    # a first guess; the library names what it needs
    ring_offsets, ring_areas, xy = _marshal.with_capacity((4 * n + 16, 2 * int(s.counts.shape[0]) + 64), attempt)
    R, V = totals[0].value, totals[1].value
    ring_offsets, ring_areas, xy = ring_offsets[:R + 1], ring_areas[:R], xy[:2 * V].reshape(V, 2)
    extra = {}
    if nest:                                                     # on the TRACED rings, before they are simplified: the guarantee is theirs
        extra["nest"] = _nest_flat(host_definition, space, rle_rings, ring_offsets, xy)
    if tolerance is not None:                                    # the same memory space: device-resident rings never leave the device
        ring_offsets, areas2, xy, src_index, V = _simplify_flat(host_definition, space, ring_offsets, xy, tolerance)
        extra.update({"areas2": areas2, "src_index": src_index})
    if flat:
        return {"rle_rings": rle_rings, "ring_offsets": ring_offsets, "ring_areas": ring_areas, "xy": xy, "n_rings": R, "n_vertices": V, **extra}
    rle_rings, ring_offsets, ring_areas, xy = (space.host(a) for a in (rle_rings, ring_offsets, ring_areas, xy))
    rings = [[[xy[ring_offsets[r]:ring_offsets[r + 1]] for r in range(rle_rings[b * slots + i], rle_rings[b * slots + i + 1])]
              for i in range(slots)] for b in range(B)]
    areas = [[ring_areas[rle_rings[b * slots + i]:rle_rings[b * slots + i + 1]] for i in range(slots)] for b in range(B)]
    if nest:
        return rings, areas, _nest_nested(extra["nest"], rle_rings, [slots] * B)
    return rings, areas


def rle_to_polygons(rles, sizes=None, device=None, flat: bool = False, tolerance=None, nest: bool = False):
    """The boundary of every mask of an RLE set as closed rings of pixel corners, traced from the runs on the GPU
    (``mrcnn_rle_to_polygons``; the geometry is defined in include/maskrcnn_hip.h).  ``rles`` as rle_decode_planes takes them: what
    merge_tiles, unite_tiles or masks_rle_source returned, or a (counts, run_offsets) pair with ``sizes``; a pair of CUDA tensors is
    traced where it lies.  Returns (rings, areas): rings[b][i] is the list of the (m, 2) int32 arrays of RLE i of image b — x then y
    per vertex, every ring, outlines and holes alike, ordered by their start vertex — and areas[b][i] their signed areas as int64:
    positive for an outline, negative for a hole.  flat=True returns the library's own arrays instead (rle_rings, ring_offsets,
    ring_areas, xy as (V, 2), n_rings, n_vertices): numpy arrays, or tensors that stay on the device when ``device`` is given or the
    pair is CUDA tensors.  ``tolerance`` (pixels; None: the traced rings as they are) hands the rings on to simplify_polygons in the
    same memory space: the rings come back simplified with the ORIGINAL pixel areas beside them, and the flat form gains areas2 and
    src_index.  ``nest=True`` adds the nesting of the rings into outlines and their holes (nest_polygons), computed in the same memory
    space on the traced rings before they are simplified — simplification keeps the rings one for one, so it indexes the simplified
    rings too: a third result, as nest_polygons returns it for the nested form, or the key "nest" of the flat form."""
    return _rle_to_polygons(False, rles, sizes, device, flat, tolerance, nest)


def rle_to_polygons_host(rles, sizes=None, flat: bool = False, tolerance=None, nest: bool = False):
    """The definition of rle_to_polygons: the sequential host code (``mrcnn_rle_to_polygons_host``, and ``mrcnn_polygons_simplify_host``
    for a tolerance, ``mrcnn_polygons_nest_host`` for nest=True), no GPU; numpy out."""
    return _rle_to_polygons(True, rles, sizes, None, flat, tolerance, nest)


# ---- changing run-length masks (mrcnn_rle_morph, mrcnn_boundary_radius) -------------------------------------------------------------------
MORPH_OPS = {"erode": _lib.MORPH_ERODE, "dilate": _lib.MORPH_DILATE, "boundary": _lib.MORPH_BOUNDARY}


def boundary_radius(h: int, w: int, ratio: float = 0.02) -> int:
    """The band width Boundary IoU takes for an h x w image (``mrcnn_boundary_radius``): max(1, round(ratio * the diagonal)), half to
    even, in double — 16 for 480 x 640 and 102 for 3072 x 4096 at the published ratio 0.02."""
    r = C.c_int32(0)
    _lib.check(_lib.lib().mrcnn_boundary_radius(int(h), int(w), float(ratio), C.byref(r)))
    return int(r.value)


def _morph_flat(host_definition, space, counts, offs, hs, ws, radii, op):
    """mrcnn_rle_morph(_host) on a flat set of ``space``: counts, run_offsets (n + 1), and host int32 arrays hs, ws, radii of n ->
    (counts, run_offsets, areas (n), bboxes (n, 4)) in the same space.  A first attempt is sized from the input's runs; if the result
    needs more, one more call with the capacity the library reported."""
    n = int(offs.shape[0]) - 1
    ptr = space.ptr
    entry = _lib.lib().mrcnn_rle_morph_host if host_definition else _lib.lib().mrcnn_rle_morph
    head = (ptr(counts), ptr(offs), n, hs.ctypes.data, ws.ctypes.data, radii.ctypes.data, int(op)) + (() if host_definition else (space.code,))
    return _marshal.rle_out(space, n, int(counts.shape[0]) + 2 * n + 2, lambda *tail: entry(*head, *tail))


def rle_rows_of(pair, sizes):
    """A (counts, run_offsets) pair of B * slots RLEs, numpy arrays or CUDA tensors, as the rows rles[b][i] = {"size": [h_b, w_b],
    "counts": uint32 runs} on the host, for ``sizes`` = [(h_b, w_b)] per image."""
    c, o = (a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a) for a in pair)
    c, B = c.view(np.uint32), len(sizes)
    slots = (len(o) - 1) // B if B else 0
    return [[{"size": [int(sizes[b][0]), int(sizes[b][1])], "counts": c[int(o[b * slots + i]):int(o[b * slots + i + 1])]} for i in range(slots)]
            for b in range(B)]


def _rle_back(s, pair_out, areas, bboxes, sizes=None):
    """(rle, areas, bboxes) of a call that returns one RLE per RLE of the set ``s``, in the form the set came in: the pair as it is, or
    host rows with areas (B, slots) and bboxes (B, slots, 4).  sizes: the (h, w) of every output plane where they are not the input's."""
    if s.pair:
        return pair_out, areas, bboxes
    host, B, slots = s.space.host, s.B, s.slots
    if sizes is None:
        rles = rle_rows_of(pair_out, s.image_sizes() if slots else [])
    else:
        c, o = host(pair_out[0]).view(np.uint32), host(pair_out[1])
        rles = [[{"size": list(sizes[k]), "counts": c[int(o[k]):int(o[k + 1])]} for k in range(b * slots, (b + 1) * slots)] for b in range(B)]
    return rles, host(areas).view(np.uint32).reshape(B, slots), host(bboxes).reshape(B, slots, 4)


def _rows_flat(s, pair_out, owner):
    """One host row per result where there is no (B, slots) grid any more: result j lies over the plane of the set's RLE owner[j]."""
    c, o = s.space.host(pair_out[0]).view(np.uint32), s.space.host(pair_out[1])
    hs, ws = s.sides()
    return [{"size": [int(hs[k]), int(ws[k])], "counts": c[int(o[j]):int(o[j + 1])]} for j, k in enumerate(owner)]


def _rle_morph(host_definition, rle, sizes, radii, op, device):
    name = "rle_morph_host" if host_definition else "rle_morph"
    op = _marshal.choice(MORPH_OPS, op, f"{name}: op {op!r} is none of {sorted(MORPH_OPS)}")
    s = _marshal.RleSet(name, rle, sizes, device, host_definition)
    B, slots, n = s.B, s.slots, s.n
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if r.size not in (1, B, n) or r.size == 0:
        raise ValueError(f"{name}: {r.size} radii for {n} RLEs of {B} sizes: one, one per size or one per RLE expected")
    if (r != np.rint(r)).any() or (np.abs(r) > 2 ** 30).any():
        raise ValueError(f"{name}: a radius is a whole number of pixels")
    r = np.ascontiguousarray(np.broadcast_to(r, (n,)) if r.size in (1, n) else np.repeat(r, slots)).astype(np.int32)
    out, out_offs, areas, bboxes = _morph_flat(host_definition, s.space, s.counts, s.offs, *s.sides(), r, op)
    return _rle_back(s, (out, out_offs), areas, bboxes)


def rle_morph(rle, sizes, radii, op, device=None):
    """A set of run-length masks eroded, dilated or cut down to its inner boundary band on the GPU, RLE in and RLE out, no plane in
    between (``mrcnn_rle_morph``; the rule is defined in include/maskrcnn_hip.h: a square structuring element of radius r, pixels
    outside the image are 0).  ``rle`` is a (counts, run_offsets) pair — numpy arrays or CUDA tensors, which are changed where they lie
    (DeviceDetections and COCOGroundTruth.to_device() hold such pairs; _merge_tiles leaves one) — with ``sizes`` = [(h, w)] per RLE or
    per image of equally many RLEs, or the rows rles[b][i] = {"size", "counts"} that masks_rle_source, merge_tiles and unite_tiles
    return (sizes may be None).  ``radii``: one radius, or one per size or per RLE, 0..1024.  ``op``: "erode", "dilate" or "boundary"
    (the mask minus its erosion).  Returns (rle, areas, bboxes): the result in the form it came in — a pair in the same memory space,
    or rows — with the set pixels and their tight boxes x, y, w, h as masks_rle_source gives them, per RLE for a pair and (B, slots)
    for rows.  The result feeds rle_to_polygons, instance_map_rle, rle_decode_planes and coco_eval as it is."""
    return _rle_morph(False, rle, sizes, radii, op, device)


def rle_morph_host(rle, sizes, radii, op):
    """The definition of rle_morph: the sequential host code (``mrcnn_rle_morph_host``), no GPU; numpy out."""
    return _rle_morph(True, rle, sizes, radii, op, None)


def _band_radii(name, rle, sizes, ratio, radius):
    if radius is not None:
        return radius
    if sizes is None:
        sizes = [row[0]["size"] for row in rle]
    return [boundary_radius(int(s[0]), int(s[1]), ratio) for s in sizes]


def rle_erode(rle, sizes, radius, device=None):
    """rle_morph(..., "erode")[0]: the masks shrunk by ``radius`` pixels, from the image border too."""
    return _rle_morph(False, rle, sizes, radius, "erode", device)[0]


def rle_dilate(rle, sizes, radius, device=None):
    """rle_morph(..., "dilate")[0]: the masks buffered by ``radius`` pixels, clipped to the image."""
    return _rle_morph(False, rle, sizes, radius, "dilate", device)[0]


def rle_boundary(rle, sizes=None, ratio: float = 0.02, radius=None, device=None):
    """rle_morph(..., "boundary")[0]: the inner band of every mask — Boundary IoU's, of width boundary_radius(h, w, ratio) per image,
    or of ``radius`` pixels when that is given."""
    return _rle_morph(False, rle, sizes, _band_radii("rle_boundary", rle, sizes, ratio, radius), "boundary", device)[0]


def rle_open(rle, sizes, radius, device=None):
    """Erode, then dilate (two calls): specks and spurs thinner than 2 * radius + 1 go, the rest keeps its size."""
    return rle_dilate(rle_erode(rle, sizes, radius, device), sizes, radius, device)


def rle_close(rle, sizes, radius, device=None):
    """Dilate, then erode (two calls): pinholes and gaps up to 2 * radius wide are filled.  The image border is 0 for both steps, so
    a mask within ``radius`` of the border loses what the dilation could not grow there."""
    return rle_erode(rle_dilate(rle, sizes, radius, device), sizes, radius, device)


def rle_erode_host(rle, sizes, radius):
    return _rle_morph(True, rle, sizes, radius, "erode", None)[0]


def rle_dilate_host(rle, sizes, radius):
    return _rle_morph(True, rle, sizes, radius, "dilate", None)[0]


def rle_boundary_host(rle, sizes=None, ratio: float = 0.02, radius=None):
    return _rle_morph(True, rle, sizes, _band_radii("rle_boundary_host", rle, sizes, ratio, radius), "boundary", None)[0]


def rle_open_host(rle, sizes, radius):
    return rle_dilate_host(rle_erode_host(rle, sizes, radius), sizes, radius)


def rle_close_host(rle, sizes, radius):
    """The definitions of rle_erode, rle_dilate, rle_boundary, rle_open and rle_close: ``mrcnn_rle_morph_host``, no GPU; numpy out."""
    return rle_erode_host(rle_dilate_host(rle, sizes, radius), sizes, radius)


# ---- cutting run-length masks into connected components (mrcnn_rle_components, mrcnn_rle_components_select) -----------------------------
COMPONENTS_OF = {"ones": _lib.COMPONENTS_OF_ONES, "zeros": _lib.COMPONENTS_OF_ZEROS}
COMPONENTS_MODES = {"merge": _lib.COMPONENTS_MERGE, "split": _lib.COMPONENTS_SPLIT}


def _components_head(s, connectivity, of):
    """the arguments the two components entries begin on"""
    of = _marshal.choice(COMPONENTS_OF, of, f"components of {of!r}: one of {sorted(COMPONENTS_OF)} expected")
    ptr, (hs, ws) = s.space.ptr, s.sides()
    return (ptr(s.counts), ptr(s.offs), s.n, hs.ctypes.data, ws.ctypes.data, int(connectivity), int(of))


def _components_flat(s, connectivity, of):
    """mrcnn_rle_components(_host) on the set: (comp_offsets (n + 1), areas, bboxes (C, 4), flags) in the set's memory space.  A first
    attempt guesses the number of components; if there are more, one more call with the capacity the library reported."""
    space, n = s.space, s.n
    ptr = space.ptr
    comp_offs = space.new(n + 1, np.int64, zero=True)
    entry = _lib.lib().mrcnn_rle_components_host if s.host_definition else _lib.lib().mrcnn_rle_components
    head = _components_head(s, connectivity, of) + (() if s.host_definition else (space.code,))

    def attempt(capacity):
        areas, bboxes, flags = space.new(capacity, np.uint32), space.new((capacity, 4), np.int32), space.new(capacity, np.uint8)
        st = entry(*head, ptr(comp_offs), ptr(areas), ptr(bboxes), ptr(flags), capacity)
        C_ = int(comp_offs[n])
        return st, C_, (comp_offs, areas[:C_], bboxes[:C_], flags[:C_])
    return _marshal.with_capacity(4 * n + 64, attempt)


def _select_flat(s, keep, connectivity, of, mode):
    """mrcnn_rle_components_select(_host) on the set with a keep mask of its space: ((counts, run_offsets), areas, bboxes, parent)."""
    mode = int(_marshal.choice(COMPONENTS_MODES, mode, f"rle_select_components: mode {mode!r} is none of {sorted(COMPONENTS_MODES)}"))
    space = s.space
    ptr = space.ptr
    keep = space.take(keep, np.uint8).reshape(-1)
    n_comps = int(keep.shape[0])
    room = n_comps if mode == _lib.COMPONENTS_SPLIT else s.n
    parent = space.new(max(1, room), np.int64)
    out_n = C.c_int64(0)
    entry = _lib.lib().mrcnn_rle_components_select_host if s.host_definition else _lib.lib().mrcnn_rle_components_select
    head = _components_head(s, connectivity, of) + ((ptr(keep) if n_comps else None), n_comps, mode) + (() if s.host_definition else (space.code,))
    out, out_offs, areas, bboxes = _marshal.rle_out(space, room, int(s.counts.shape[0]) + 2 * room + 2,
                                                    lambda *tail: entry(*head, *tail, ptr(parent), C.byref(out_n)), written=lambda: int(out_n.value))
    return (out, out_offs), areas, bboxes, parent[:int(out_n.value)]


def _rle_components(host_definition, rle, sizes, connectivity, of, device):
    s = _marshal.RleSet("rle_components_host" if host_definition else "rle_components", rle, sizes, device, host_definition)
    return _components_flat(s, connectivity, of)


def rle_components(rle, sizes=None, connectivity=4, of="ones", device=None):
    """The connected components of every mask of an RLE set, labelled and measured on the GPU from the runs, no plane in between
    (``mrcnn_rle_components``; the rule is defined in include/maskrcnn_hip.h).  ``rle`` in the forms rle_morph takes: a (counts,
    run_offsets) pair — numpy arrays or CUDA tensors, labelled where they lie, tensors out — with ``sizes``, or rows.  ``of``: "ones"
    labels the set pixels with ``connectivity`` (4 or 8), "zeros" the background with the dual connectivity, so that at connectivity 4
    the zero components that do not touch the border are the holes rle_to_polygons traces.  Returns (comp_offsets, areas, bboxes,
    flags): RLE k (b * slots + i for rows) owns the components comp_offsets[k]:comp_offsets[k + 1], numbered by their first pixel in
    column-major order; per component its pixels, its tight box x, y, w, h and flags & 1 = it touches the image border."""
    return _rle_components(False, rle, sizes, connectivity, of, device)


def rle_components_host(rle, sizes=None, connectivity=4, of="ones"):
    """The definition of rle_components: the sequential host code (``mrcnn_rle_components_host``), no GPU; numpy out."""
    return _rle_components(True, rle, sizes, connectivity, of, None)


def _rle_select(host_definition, rle, sizes, keep, connectivity, of, mode, device, s=None):
    s = s or _marshal.RleSet("rle_select_components_host" if host_definition else "rle_select_components", rle, sizes, device, host_definition)
    pair, areas, bboxes, parent = _select_flat(s, keep, connectivity, of, mode)
    if COMPONENTS_MODES.get(mode, mode) != _lib.COMPONENTS_SPLIT:
        return _rle_back(s, pair, areas, bboxes)
    if s.pair:
        return pair, areas, bboxes, parent
    host = s.space.host
    par = host(parent)
    return _rows_flat(s, pair, par), host(areas).view(np.uint32), host(bboxes), par


def rle_select_components(rle, sizes, keep, connectivity=4, of="ones", mode="merge", device=None):
    """A set of run-length masks with some of its connected components dropped, or cut into its components, on the GPU
    (``mrcnn_rle_components_select``).  ``keep``: one flag per component in rle_components' order (numpy or a CUDA tensor; it must
    hold exactly as many entries as the set has components).  mode="merge": the same RLEs come back — the pixels of a dropped
    component take the other value, so of="ones" clears specks and of="zeros" fills holes — as (rle, areas, bboxes) in the form
    rle_morph returns.  mode="split" (of="ones" only): one RLE per kept component over its parent's plane, as ((counts, run_offsets),
    areas, bboxes, parent) for a pair — parent[j] = the RLE it was cut from — or (rows, areas, bboxes, parent) with one row per
    component for rows."""
    return _rle_select(False, rle, sizes, keep, connectivity, of, mode, device)


def rle_select_components_host(rle, sizes, keep, connectivity=4, of="ones", mode="merge"):
    """The definition of rle_select_components: the sequential host code (``mrcnn_rle_components_select_host``), no GPU; numpy out."""
    return _rle_select(True, rle, sizes, keep, connectivity, of, mode, None)


def _largest_mask(comp_offs, areas, m):
    """keep flags of the m largest components of every RLE, ties to the earlier component; numpy arrays or tensors, computed where they lie"""
    if isinstance(areas, np.ndarray):
        per = np.diff(comp_offs)
        owner = np.repeat(np.arange(len(per)), per)
        order = np.lexsort((np.arange(len(areas)), -areas.astype(np.int64), owner))
        keep = np.zeros(len(areas), np.uint8)
        keep[order] = (np.arange(len(areas)) - comp_offs[:-1][owner[order]]) < m
        return keep
    import torch
    per = comp_offs[1:] - comp_offs[:-1]
    owner = torch.repeat_interleave(torch.arange(per.shape[0], device=areas.device), per)
    by_area = torch.sort(-areas.to(torch.int64), stable=True).indices          # ties keep their order
    order = by_area[torch.sort(owner[by_area], stable=True).indices]
    keep = torch.zeros(areas.shape[0], dtype=torch.uint8, device=areas.device)
    keep[order] = ((torch.arange(areas.shape[0], device=areas.device) - comp_offs[:-1][owner[order]]) < m).to(torch.uint8)
    return keep


def _filter(host_definition, name, rle, sizes, connectivity, of, mode, device, choose):
    """label, build the keep mask where the measures lie (choose(comp_offsets, areas, flags)), select"""
    s = _marshal.RleSet(name, rle, sizes, device, host_definition)
    comp_offs, areas, _, flags = _components_flat(s, connectivity, of)
    if isinstance(areas, np.ndarray):
        areas = areas.astype(np.int64)
    return _rle_select(host_definition, rle, sizes, choose(comp_offs, areas, flags), connectivity, of, mode, device, s=s)


def _remove_small(host_definition, rle, sizes, min_area, connectivity, device):
    return _filter(host_definition, "rle_remove_small", rle, sizes, connectivity, "ones", "merge", device, lambda o, a, f: a >= int(min_area))[0]


def _keep_largest(host_definition, rle, sizes, m, connectivity, device):
    return _filter(host_definition, "rle_keep_largest", rle, sizes, connectivity, "ones", "merge", device, lambda o, a, f: _largest_mask(o, a, int(m)))[0]


def _fill_holes(host_definition, rle, sizes, max_area, connectivity, device):
    choose = (lambda o, a, f: (f & 1) != 0) if max_area is None else (lambda o, a, f: ((f & 1) != 0) | (a > int(max_area)))
    return _filter(host_definition, "rle_fill_holes", rle, sizes, connectivity, "zeros", "merge", device, choose)[0]


def _split_components(host_definition, rle, sizes, min_area, connectivity, device):
    out = _filter(host_definition, "rle_split_components", rle, sizes, connectivity, "ones", "split", device, lambda o, a, f: a >= int(min_area))
    return out[0], out[3]


def rle_remove_small(rle, sizes, min_area, connectivity=4, device=None):
    """The masks without their specks: the components of ones with fewer than ``min_area`` pixels are cleared, everything else keeps
    its outline (rle_components, then rle_select_components; the keep mask is computed where the measures lie).  Returns the rle in
    the form it came in."""
    return _remove_small(False, rle, sizes, min_area, connectivity, device)


def rle_keep_largest(rle, sizes, m=1, connectivity=4, device=None):
    """The ``m`` largest components of every mask, the rest cleared; of equally large components the earlier one stays."""
    return _keep_largest(False, rle, sizes, m, connectivity, device)


def rle_fill_holes(rle, sizes=None, max_area=None, connectivity=4, device=None):
    """The masks with their holes filled: the components of zeros (dual connectivity) that do not touch the image border are set —
    all of them, or with ``max_area`` only those of at most that many pixels."""
    return _fill_holes(False, rle, sizes, max_area, connectivity, device)


def rle_split_components(rle, sizes, min_area=0, connectivity=4, device=None):
    """Every mask cut into its components of at least ``min_area`` pixels: (split set, parent) — one RLE per component over its
    parent's plane, a (counts, run_offsets) pair for a pair and one row per component for rows; parent[j] = the RLE it was cut from."""
    return _split_components(False, rle, sizes, min_area, connectivity, device)


def rle_remove_small_host(rle, sizes, min_area, connectivity=4):
    return _remove_small(True, rle, sizes, min_area, connectivity, None)


def rle_keep_largest_host(rle, sizes, m=1, connectivity=4):
    return _keep_largest(True, rle, sizes, m, connectivity, None)


def rle_fill_holes_host(rle, sizes=None, max_area=None, connectivity=4):
    return _fill_holes(True, rle, sizes, max_area, connectivity, None)


def rle_split_components_host(rle, sizes, min_area=0, connectivity=4):
    """The definitions of rle_remove_small, rle_keep_largest, rle_fill_holes and rle_split_components: the _host entries, no GPU; numpy out."""
    return _split_components(True, rle, sizes, min_area, connectivity, None)


# ---- combining run-length masks (mrcnn_rle_combine) -----------------------------------------------------------------------------------------
COMBINE_OPS = {"or": _lib.RLE_OR, "and": _lib.RLE_AND, "xor": _lib.RLE_XOR, "diff": _lib.RLE_DIFF}


def _groups_of(name, groups):
    """(group_offsets, members) as int64 host arrays: from a list of index lists, or from a tuple (offsets, members)"""
    if isinstance(groups, tuple):
        if len(groups) != 2:
            raise ValueError(f"{name}: groups is a list of index lists or an (offsets, members) pair")
        offs, mem = (_marshal.HOST.take(a, np.int64).reshape(-1) for a in groups)
    else:
        rows = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
        offs = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
        mem = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    if offs.size == 0:
        raise ValueError(f"{name}: group offsets hold one entry more than there are groups")
    return offs, (mem if mem.size else np.zeros(1, np.int64))


def _combine_flat(host_definition, space, counts, offs, hs, ws, goffs, mem, op):
    """mrcnn_rle_combine(_host) on a flat set of ``space`` — counts, run_offsets (n + 1), host int32 arrays hs, ws of n — and host int64
    group tables -> (counts, run_offsets (G + 1), areas (G), bboxes (G, 4)) in the same space.  A first attempt is sized from the
    input's runs; if the result needs more, one more call with the capacity the library reported."""
    n, G = int(offs.shape[0]) - 1, int(goffs.shape[0]) - 1
    ptr = space.ptr
    entry = _lib.lib().mrcnn_rle_combine_host if host_definition else _lib.lib().mrcnn_rle_combine
    head = (ptr(counts), ptr(offs), n, hs.ctypes.data, ws.ctypes.data, goffs.ctypes.data, mem.ctypes.data, G, int(op)) + (() if host_definition else (space.code,))
    return _marshal.rle_out(space, G, int(counts.shape[0]) + 2 * G + 2, lambda *tail: entry(*head, *tail))


def _rle_combine(host_definition, rle, sizes, groups, op, device, name=None):
    name = name or ("rle_combine_host" if host_definition else "rle_combine")
    op = _marshal.choice(COMBINE_OPS, op, f"{name}: op {op!r} is none of {sorted(COMBINE_OPS)}")
    s = _marshal.RleSet(name, rle, sizes, device, host_definition)
    goffs, mem = _groups_of(name, groups)
    out, out_offs, areas, bboxes = _combine_flat(host_definition, s.space, s.counts, s.offs, *s.sides(), goffs, mem, op)
    if s.pair:
        return (out, out_offs), areas, bboxes
    return _rows_flat(s, (out, out_offs), mem[goffs[:-1]]), s.space.host(areas).view(np.uint32), s.space.host(bboxes)


def rle_combine(rle, sizes, groups, op, device=None):
    """Run-length masks combined on the GPU, RLE in and RLE out, no plane in between (``mrcnn_rle_combine``; the rule is defined in
    include/maskrcnn_hip.h) — the counterpart of pycocotools' mask.merge.  ``rle`` in the forms rle_morph takes: a (counts,
    run_offsets) pair — numpy arrays or CUDA tensors, combined where they lie — with ``sizes`` = [(h, w)] per RLE or per image of
    equally many RLEs, or the rows rles[b][i] = {"size", "counts"} (RLE k = b * slots + i; sizes may be None).  ``groups``: a list of
    index lists, or a tuple (offsets, members) of int64 arrays; group g combines the RLEs members[offsets[g]:offsets[g + 1]] in that
    order over the plane of the first one — all of one size, none empty; an RLE may serve any number of groups, and one group more
    than once.  ``op``: "or" (set in some member), "and" (in every member), "xor" (in an odd number; a member listed twice counts
    twice) or "diff" (in the first and in none of the others).  Returns (rle, areas, bboxes), one canonical RLE per group: a pair in
    the same memory space for a pair (a resident pair stays resident), else a list of rows {"size", "counts"}; with the set pixels
    and their tight boxes x, y, w, h per group.  The result feeds rle_to_polygons, instance_map_rle, rle_decode_planes and coco_eval
    as it is.  Not here: votes (at least m of K), planes of different sizes in one group (rle_place brings them into one frame
    first), group tables on the device, the complement (XOR with the full mask [0, h*w])."""
    return _rle_combine(False, rle, sizes, groups, op, device)


def rle_combine_host(rle, sizes, groups, op):
    """The definition of rle_combine: the sequential host code (``mrcnn_rle_combine_host``), no GPU; numpy out."""
    return _rle_combine(True, rle, sizes, groups, op, None)


def _cat(a, b):
    if isinstance(a, np.ndarray):
        return np.concatenate((a, b))
    import torch
    return torch.cat((a, b))


def _pairwise(host_definition, name, rle, sizes, other, op, device):
    """A[k] op B[k] for two sets of equally many RLEs of equal sizes, in the form A came in: rows (B, slots) or a pair"""
    if other is None:
        raise ValueError(f"{name}: groups, or a second set ``other`` to combine pairwise, expected")
    A = _marshal.RleSet(name, rle, sizes, device, host_definition)
    O = _marshal.RleSet(name, other, sizes, A.space.device, host_definition)
    (hs, ws), (hs2, ws2) = A.sides(), O.sides()
    if (O.B, O.slots) != (A.B, A.slots) or (hs2 != hs).any() or (ws2 != ws).any():
        raise ValueError(f"{name}: the two sets differ in their number of RLEs or in their sizes")
    n, (ca, oa), (cb, ob) = A.n, (A.counts, A.offs), (O.counts, O.offs)
    a0, a1, b0, b1 = int(oa[0]), int(oa[n]), int(ob[0]), int(ob[n])
    counts = _marshal.addressable(_cat(ca[a0:a1], cb[b0:b1]))             # the two sets behind each other: B's RLE k is RLE n + k
    offs = _cat(oa - a0, ob[1:] - b0 + (a1 - a0))
    goffs = 2 * np.arange(n + 1, dtype=np.int64)
    mem = np.stack((np.arange(n, dtype=np.int64), n + np.arange(n, dtype=np.int64)), 1).reshape(-1)
    out, out_offs, _, _ = _combine_flat(host_definition, A.space, counts, offs, np.tile(hs, 2), np.tile(ws, 2), goffs,
                                        mem if n else np.zeros(1, np.int64), COMBINE_OPS[op])
    if A.pair:
        return (out, out_offs)
    return rle_rows_of((out, out_offs), A.image_sizes() if A.slots else [])      # (areas and boxes are not asked for: not read back)


def _algebra(host_definition, name, rle, sizes, groups, other, op, device):
    if groups is None:
        return _pairwise(host_definition, name, rle, sizes, other, op, device)
    if other is not None:
        raise ValueError(f"{name}: either groups over one set or a second set to combine pairwise, not both")
    return _rle_combine(host_definition, rle, sizes, groups, op, device, name)[0]


def rle_union(rle, sizes=None, groups=None, other=None, device=None):
    """rle_combine(..., "or")[0]: per group the pixels set in at least one member.  With ``groups`` = None the sets ``rle`` and
    ``other`` — equally many RLEs of equal sizes, in the same form — are combined pairwise, rle[k] with other[k], and the result
    comes back in the form of ``rle`` (rows (B, slots) or a pair): masking with a region."""
    return _algebra(False, "rle_union", rle, sizes, groups, other, "or", device)


def rle_intersection(rle, sizes=None, groups=None, other=None, device=None):
    """rle_combine(..., "and")[0]: the pixels set in every member; pairwise with ``other`` like rle_union."""
    return _algebra(False, "rle_intersection", rle, sizes, groups, other, "and", device)


def rle_xor(rle, sizes=None, groups=None, other=None, device=None):
    """rle_combine(..., "xor")[0]: the pixels set in an odd number of members; pairwise with ``other`` like rle_union."""
    return _algebra(False, "rle_xor", rle, sizes, groups, other, "xor", device)


def rle_difference(rle, sizes=None, groups=None, other=None, device=None):
    """rle_combine(..., "diff")[0]: the pixels of the first member that no other member has; pairwise (rle[k] minus other[k]) with
    ``other`` like rle_union."""
    return _algebra(False, "rle_difference", rle, sizes, groups, other, "diff", device)


def rle_union_host(rle, sizes=None, groups=None, other=None):
    return _algebra(True, "rle_union_host", rle, sizes, groups, other, "or", None)


def rle_intersection_host(rle, sizes=None, groups=None, other=None):
    return _algebra(True, "rle_intersection_host", rle, sizes, groups, other, "and", None)


def rle_xor_host(rle, sizes=None, groups=None, other=None):
    return _algebra(True, "rle_xor_host", rle, sizes, groups, other, "xor", None)


def rle_difference_host(rle, sizes=None, groups=None, other=None):
    """The definitions of rle_union, rle_intersection, rle_xor and rle_difference: ``mrcnn_rle_combine_host``, no GPU; numpy out."""
    return _algebra(True, "rle_difference_host", rle, sizes, groups, other, "diff", None)


def drawn_rows(det_src, sizes, min_score: float = 0.0) -> np.ndarray:
    """Which rows mrcnn_instance_map_rle draws: (B, slots) bool for det_src (B, slots, 6), numpy or a CUDA tensor (read back), and
    ``sizes`` = [(h_b, w_b)] — score > min_score, score > 0 and a non-empty pixel box, the box rounded as csrc/draw_rule.h rounds it:
    half-to-even of y * (h - 1) in double, + 1 on the far edge, a NaN 0, held to +-2^20."""
    det = np.asarray(det_src.cpu().numpy() if hasattr(det_src, "is_cuda") else det_src, dtype=np.float32)
    hs, ws = sizes_of(sizes)
    d = det.astype(np.float64)
    h1, w1 = (hs.astype(np.float64) - 1.0)[:, None], (ws.astype(np.float64) - 1.0)[:, None]
    with np.errstate(invalid="ignore"):
        box = [d[..., 0] * h1, d[..., 1] * w1, d[..., 2] * h1 + 1.0, d[..., 3] * w1 + 1.0]
    y1, x1, y2, x2 = (np.rint(np.clip(np.where(np.isnan(v), 0.0, v), -1048576.0, 1048576.0)) for v in box)
    score = det[..., 5]
    return (score > np.float32(min_score)) & (score > np.float32(0)) & (y2 > y1) & (x2 > x1)


def _rle_disjoint(host_definition, det_src, rle, sizes, min_score, device):
    name = "rle_disjoint_host" if host_definition else "rle_disjoint"
    if device is None and not host_definition and _marshal.pair_device(rle) is None:
        device = Space(det_src).device                           # the rows say where the call runs, as for instance_map_rle
    s = _marshal.RleSet(name, rle, sizes, device, host_definition)
    B, slots = s.B, s.slots
    det = np.asarray(det_src.cpu().numpy() if hasattr(det_src, "is_cuda") else det_src, dtype=np.float32)
    if det.ndim != 3 or det.shape[0] != B or det.shape[1] != slots or det.shape[2] != 6:
        raise ValueError(f"{name}: det_src {tuple(det.shape)} does not go with {B} images of {slots} RLEs: ({B}, {slots}, 6) expected")
    drawn = drawn_rows(det, s.image_sizes(), min_score) if slots else np.zeros((B, 0), bool)
    groups = []
    for b in range(B):
        above = []                                               # the drawn rows before row i
        for i in range(slots):
            k = b * slots + i
            groups.append([k] + above if drawn[b, i] else [k, k])                   # an undrawn row minus itself: the empty mask
            if drawn[b, i]:
                above = above + [k]
    goffs, mem = _groups_of(name, groups)
    out, out_offs, areas, bboxes = _combine_flat(host_definition, s.space, s.counts, s.offs, *s.sides(), goffs, mem, _lib.RLE_DIFF)
    return _rle_back(s, (out, out_offs), areas, bboxes)


def rle_disjoint(det_src, rle, sizes=None, min_score: float = 0.0, device=None):
    """The masks of a detection set made disjoint on the GPU (one ``mrcnn_rle_combine`` call): per image, row i keeps the pixels no
    drawn row j < i has — the pixels where instance_map_rle's map equals i — and an undrawn row becomes the empty mask.  "Drawn" is
    instance_map_rle's rule (drawn_rows), evaluated from ``det_src`` (B, slots, 6) on the host (a small read-back for a CUDA tensor).
    ``rle`` as instance_map_rle takes it: rows, or a (counts, run_offsets) pair with ``sizes``; a pair of CUDA tensors is used in
    place.  Returns (rle, areas, bboxes) as rle_morph returns them, rows (B, slots) or a pair in the same memory space; the areas are
    instance_map_rle's visible areas.  Footprints for a GIS layer, a GeoJSON file or a COCO result without overlaps."""
    return _rle_disjoint(False, det_src, rle, sizes, min_score, device)


def rle_disjoint_host(det_src, rle, sizes=None, min_score: float = 0.0):
    """The definition of rle_disjoint: the sequential host code (``mrcnn_rle_combine_host``), no GPU; numpy out."""
    return _rle_disjoint(True, det_src, rle, sizes, min_score, None)


# ---- moving run-length masks to another pixel grid (mrcnn_rle_transform) ------------------------------------------------------------------
XF_TRANSPOSE = _lib.XF_TRANSPOSE


def _transform_flat(host_definition, space, counts, offs, hs, ws, ohs, ows, xf):
    """mrcnn_rle_transform(_host) on a flat set of ``space`` — counts, run_offsets (n + 1), host int32 arrays hs, ws, ohs, ows of n and
    the host int64 records xf (n, 8) -> (counts, run_offsets, areas (n), bboxes (n, 4)) in the same space.  A first attempt is sized
    from the input's runs; if the result needs more, one more call with the capacity the library reported."""
    n = int(offs.shape[0]) - 1
    ptr = space.ptr
    entry = _lib.lib().mrcnn_rle_transform_host if host_definition else _lib.lib().mrcnn_rle_transform
    head = (ptr(counts), ptr(offs), n, hs.ctypes.data, ws.ctypes.data, ohs.ctypes.data, ows.ctypes.data, xf.ctypes.data) + (() if host_definition else (space.code,))
    return _marshal.rle_out(space, n, int(counts.shape[0]) + 2 * n + 2, lambda *tail: entry(*head, *tail))


def _per_rle(name, what, a, width, B, slots, dtype=np.int64):
    """``a`` — one row of ``width`` whole numbers, one per size or one per RLE — as an (n, width) array, one row per RLE"""
    n = B * slots
    v = np.asarray(a.cpu().numpy() if hasattr(a, "is_cuda") else a, dtype=np.float64)
    if v.size == 0 or v.size % width or v.size // width not in (1, B, n):
        raise ValueError(f"{name}: {what} holds {v.size} numbers for {n} RLEs of {B} sizes: {width} each for all, per size or per RLE expected")
    if (v != np.rint(v)).any() or (np.abs(v) > 2.0 ** 62).any():
        raise ValueError(f"{name}: {what} holds whole numbers")
    v = v.reshape(-1, width)
    v = np.repeat(v, slots, 0) if (len(v) == B and B != n) else np.broadcast_to(v, (n, width))
    return np.ascontiguousarray(v).astype(dtype)


def _xf_call(host_definition, name, rle, sizes, device, make):
    """One transform call: ``make(hs, ws, per)`` -> (xf (n, 8), out sizes (n, 2) as (h, w)) from the planes' sides per RLE, with
    per(what, a, width) = _per_rle of this set.  Returns (rle, areas, boxes, sizes) in the form ``rle`` came in."""
    s = _marshal.RleSet(name, rle, sizes, device, host_definition)
    B, slots, n = s.B, s.slots, s.n
    xf, osz = np.zeros((1, 8), np.int64), np.ones((1, 2), np.int64)          # (no RLE: nothing is read)
    if n:
        hs, ws = s.sides()
        xf, osz = make(hs.astype(np.int64), ws.astype(np.int64), lambda what, a, width: _per_rle(name, what, a, width, B, slots))
        xf, osz = np.ascontiguousarray(xf, dtype=np.int64).reshape(n, 8), np.asarray(osz, dtype=np.int64).reshape(n, 2)
    if n and ((osz < 1).any() or (osz > 32767).any()):
        raise ValueError(f"{name}: an output plane of {osz[((osz < 1) | (osz > 32767)).any(1)][0].tolist()}: height and width must lie in 1..32767")
    ohs, ows = np.ascontiguousarray(osz[:, 0], dtype=np.int32), np.ascontiguousarray(osz[:, 1], dtype=np.int32)
    out, out_offs, areas, bboxes = _transform_flat(host_definition, s.space, s.counts, s.offs, *s.sides(), ohs, ows, xf)
    per = [(int(h), int(w)) for h, w in zip(ohs[:n], ows[:n])]
    uniform = slots > 0 and all(per[b * slots + i] == per[b * slots] for b in range(B) for i in range(slots))
    new_sizes = [per[b * slots] for b in range(B)] if uniform else per      # per image where every RLE of an image got the same plane
    return (*_rle_back(s, (out, out_offs), areas, bboxes, sizes=per), new_sizes)


def _records(flags, ax, bx, dx, ay, by, dy):
    """(n, 8) int64 records from per-RLE columns (scalars broadcast)"""
    n = max(np.size(v) for v in (flags, ax, bx, dx, ay, by, dy))
    return np.stack([np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)) for v in (flags, ax, bx, dx, ay, by, dy, 0)], 1)


def _rle_transform(host_definition, rle, sizes, xf, out_sizes, device, name=None):
    name = name or ("rle_transform_host" if host_definition else "rle_transform")
    return _xf_call(host_definition, name, rle, sizes, device, lambda hs, ws, per: (per("xf", xf, 8), per("out_sizes", out_sizes, 2)))


def rle_transform(rle, sizes, xf, out_sizes, device=None):
    """Run-length masks moved to another pixel grid on the GPU, RLE in and RLE out, no plane in between (``mrcnn_rle_transform``; the
    rule is defined in include/maskrcnn_hip.h).  ``rle`` in the forms rle_morph takes: a (counts, run_offsets) pair — numpy arrays or
    CUDA tensors, moved where they lie — with ``sizes`` = [(h, w)] per RLE or per image of equally many RLEs, or the rows rles[b][i] =
    {"size", "counts"} (sizes may be None).  ``xf``: records [flags, ax, bx, dx, ay, by, dy, 0], one for all, one per size or one per
    RLE; the output pixel (X, Y) is the source pixel (floor((ax*X + bx)/dx), floor((ay*Y + by)/dy)) — the two swapped when flags is
    XF_TRANSPOSE — and 0 where that lies outside the plane.  ``out_sizes``: the output planes (h, w), given the same three ways.
    Returns (rle, areas, boxes, sizes): one canonical RLE per input in the form it came in — a pair in the same memory space (a
    resident pair stays resident), or rows — the set pixels and their tight boxes x, y, w, h (per RLE for a pair, (B, slots) for rows),
    and the new sizes to pass on with a pair: per image where every RLE of an image got the same plane, else per RLE.  rle_crop,
    rle_place, rle_flip, rle_transpose, rle_rot90 and rle_resize write the records for the usual cases.  Not here: rotation by other
    angles, affine or projective warps, anti-aliased resampling, moving the detection boxes along, composing two records."""
    return _rle_transform(False, rle, sizes, xf, out_sizes, device)


def rle_transform_host(rle, sizes, xf, out_sizes):
    """The definition of rle_transform: the sequential host code (``mrcnn_rle_transform_host``), no GPU; numpy out."""
    return _rle_transform(True, rle, sizes, xf, out_sizes, None)


def _rle_crop(host_definition, rle, sizes, windows, device):
    def make(hs, ws, per):
        win = per("windows", windows, 4)
        return _records(0, 1, win[:, 0], 1, 1, win[:, 1], 1), win[:, [3, 2]]
    return _xf_call(host_definition, "rle_crop_host" if host_definition else "rle_crop", rle, sizes, device, make)


def _rle_place(host_definition, rle, sizes, origins, frame_sizes, device):
    def make(hs, ws, per):
        at = per("origins", origins, 2)
        return _records(0, 1, -at[:, 0], 1, 1, -at[:, 1], 1), per("frame_sizes", frame_sizes, 2)
    return _xf_call(host_definition, "rle_place_host" if host_definition else "rle_place", rle, sizes, device, make)


def _rle_flip(host_definition, rle, sizes, horizontal, vertical, device):
    def make(hs, ws, per):
        fx, fy = bool(horizontal), bool(vertical)
        return _records(0, -1 if fx else 1, (ws - 1) if fx else 0 * ws, 1, -1 if fy else 1, (hs - 1) if fy else 0 * hs, 1), np.stack((hs, ws), 1)
    return _xf_call(host_definition, "rle_flip_host" if host_definition else "rle_flip", rle, sizes, device, make)


def _rle_rot90(host_definition, rle, sizes, k, device, name):
    def make(hs, ws, per):
        turn = int(k) % 4
        if turn == 0 and name.startswith("rle_rot90"):
            return _records(0, 1, 0 * ws, 1, 1, 0, 1), np.stack((hs, ws), 1)
        if turn == 0:                                            # rle_transpose: Out[Y, X] = P[X, Y]
            return _records(XF_TRANSPOSE, 1, 0 * ws, 1, 1, 0, 1), np.stack((ws, hs), 1)
        if turn == 1:                                            # Out[Y, X] = P[X, w-1-Y]
            return _records(XF_TRANSPOSE, 1, 0 * ws, 1, -1, ws - 1, 1), np.stack((ws, hs), 1)
        if turn == 2:                                            # Out[Y, X] = P[h-1-Y, w-1-X]
            return _records(0, -1, ws - 1, 1, -1, hs - 1, 1), np.stack((hs, ws), 1)
        return _records(XF_TRANSPOSE, -1, hs - 1, 1, 1, 0, 1), np.stack((ws, hs), 1)       # Out[Y, X] = P[h-1-X, Y]
    return _xf_call(host_definition, name, rle, sizes, device, make)


RESIZE_RULES = ("center", "floor")


def _rle_resize(host_definition, rle, sizes, out_sizes, rule, device):
    name = "rle_resize_host" if host_definition else "rle_resize"
    if rule not in RESIZE_RULES:
        raise ValueError(f"{name}: rule {rule!r} is none of {list(RESIZE_RULES)}")

    def make(hs, ws, per):
        osz = per("out_sizes", out_sizes, 2)
        oh, ow = np.maximum(osz[:, 0], 1), np.maximum(osz[:, 1], 1)          # (a side below 1 is refused by its own message)
        if rule == "center":                                     # src = floor((2X + 1) * w / (2W'))
            return _records(0, 2 * ws, ws, 2 * ow, 2 * hs, hs, 2 * oh), osz
        return _records(0, ws, 0, ow, hs, 0, oh), osz            # src = floor(X * w / W')
    return _xf_call(host_definition, name, rle, sizes, device, make)


def rle_crop(rle, sizes, windows, device=None):
    """The masks cut down to a window (rle_transform with a = 1, d = 1, b = (x, y)).  ``windows``: (x, y, w, h), one for all, one per
    size or one per RLE; a window may reach outside the plane, and that part is 0.  Returns (rle, areas, boxes, sizes) as
    rle_transform does; the new planes are the windows'."""
    return _rle_crop(False, rle, sizes, windows, device)


def rle_place(rle, sizes, origins, frame_sizes, device=None):
    """The masks put into a larger (or any other) frame with their plane's corner at ``origins`` = (x0, y0) — the inverse of rle_crop,
    and what brings sets from planes of different sizes into one frame for rle_combine.  ``frame_sizes``: (h, w); both one for all,
    one per size or one per RLE.  What falls outside the frame is cut.  Returns (rle, areas, boxes, sizes) as rle_transform does."""
    return _rle_place(False, rle, sizes, origins, frame_sizes, device)


def rle_flip(rle, sizes=None, horizontal=False, vertical=False, device=None):
    """The masks mirrored left-right (``horizontal``), top-bottom (``vertical``) or both: np.flip along axis 1 / axis 0."""
    return _rle_flip(False, rle, sizes, horizontal, vertical, device)


def rle_transpose(rle, sizes=None, device=None):
    """The masks transposed: plane.T, an h x w plane becomes w x h."""
    return _rle_rot90(False, rle, sizes, 0, device, "rle_transpose")


def rle_rot90(rle, sizes=None, k=1, device=None):
    """The masks rotated by k quarter turns in np.rot90's sense (k = 1: counterclockwise on the screen)."""
    return _rle_rot90(False, rle, sizes, k, device, "rle_rot90")


def rle_resize(rle, sizes, out_sizes, rule="center", device=None):
    """The masks resized to ``out_sizes`` = (h, w) — one for all, one per size or one per RLE — by nearest neighbour: ``rule`` =
    "center" reads src = floor((2X + 1) * w / (2W')), the pixel under the output pixel's centre; "floor" reads floor(X * w / W')."""
    return _rle_resize(False, rle, sizes, out_sizes, rule, device)


def rle_crop_host(rle, sizes, windows):
    return _rle_crop(True, rle, sizes, windows, None)


def rle_place_host(rle, sizes, origins, frame_sizes):
    return _rle_place(True, rle, sizes, origins, frame_sizes, None)


def rle_flip_host(rle, sizes=None, horizontal=False, vertical=False):
    return _rle_flip(True, rle, sizes, horizontal, vertical, None)


def rle_transpose_host(rle, sizes=None):
    return _rle_rot90(True, rle, sizes, 0, None, "rle_transpose_host")


def rle_rot90_host(rle, sizes=None, k=1):
    return _rle_rot90(True, rle, sizes, k, None, "rle_rot90_host")


def rle_resize_host(rle, sizes, out_sizes, rule="center"):
    """The definitions of rle_crop, rle_place, rle_flip, rle_transpose, rle_rot90 and rle_resize: ``mrcnn_rle_transform_host``, no GPU;
    numpy out."""
    return _rle_resize(True, rle, sizes, out_sizes, rule, None)


# ---- measuring run-length masks (mrcnn_rle_measure, mrcnn_rle_convex_hull) ------------------------------------------------------------------
MEASURE_WORDS = _lib.MEASURE_WORDS
HULL_LDS_COLUMNS = _lib.HULL_LDS_COLUMNS          # MRCNN_HULL_LDS_COLUMNS: a hull of more vertex columns (w + 1) is built in global scratch


def _measure_flat(host_definition, space, counts, offs, hs, ws):
    """mrcnn_rle_measure(_host) on a flat set of ``space`` -> measures (n, 7) int64 in the same space"""
    n = int(offs.shape[0]) - 1
    out = space.new((max(1, n), MEASURE_WORDS), np.int64)
    ptr = space.ptr
    head = (ptr(counts), ptr(offs), n, hs.ctypes.data, ws.ctypes.data)
    if host_definition:
        _lib.check(_lib.lib().mrcnn_rle_measure_host(*head, ptr(out)))
    else:
        _lib.check(_lib.lib().mrcnn_rle_measure(*head, space.code, ptr(out)))
    return out[:n]


def _hull_flat(host_definition, space, counts, offs, hs, ws):
    """mrcnn_rle_convex_hull(_host) on a flat set of ``space`` -> (hull_offsets (n + 1), xy (V, 2), areas2 (n), obb (n, 8)) in the same
    space.  A first attempt guesses the number of vertices; if there are more, one more call with the capacity the library reported."""
    n = int(offs.shape[0]) - 1
    ptr = space.ptr
    hull_offs, areas2, obb = space.new(n + 1, np.int64, zero=True), space.new(max(1, n), np.int64), space.new((max(1, n), 8), np.int64)
    entry = _lib.lib().mrcnn_rle_convex_hull_host if host_definition else _lib.lib().mrcnn_rle_convex_hull
    head = (ptr(counts), ptr(offs), n, hs.ctypes.data, ws.ctypes.data) + (() if host_definition else (space.code,))
    nv = C.c_int64(0)

    def attempt(capacity):
        xy = space.new((max(1, capacity), 2), np.int32)
        st = entry(*head, ptr(hull_offs), ptr(areas2), ptr(obb), ptr(xy), C.byref(nv), capacity)
        return st, int(nv.value), xy[:int(nv.value)]
    return hull_offs, _marshal.with_capacity(32 * n + 64, attempt), areas2[:n], obb[:n]


def _rle_measure(host_definition, rle, sizes, device):
    s = _marshal.RleSet("rle_measure_host" if host_definition else "rle_measure", rle, sizes, device, host_definition)
    return _measure_flat(host_definition, s.space, s.counts, s.offs, *s.sides())


def rle_measure(rle, sizes=None, device=None):
    """The moments and the perimeter of every mask of an RLE set, on the GPU from the runs, no plane in between (``mrcnn_rle_measure``;
    the rule is defined in include/maskrcnn_hip.h).  ``rle`` in the forms rle_morph takes: a (counts, run_offsets) pair — numpy arrays
    or CUDA tensors, measured where they lie, a tensor out — with ``sizes``, or rows.  Returns measures (n, 7) int64, RLE k = b * slots
    + i for rows: [S1, Sx, Sy, Sxx, Sxy, Syy, perimeter] over the set pixels with pixel indices (x, y); perimeter counts the unit edges
    between a set pixel and an unset one or the outside, the total edge length of rle_to_polygons' rings.  Central moments need more
    than 64 bits: rle_region_props takes them in Python ints."""
    return _rle_measure(False, rle, sizes, device)


def rle_measure_host(rle, sizes=None):
    """The definition of rle_measure: the sequential host code (``mrcnn_rle_measure_host``), no GPU; numpy out."""
    return _rle_measure(True, rle, sizes, None)


def _rle_convex_hull(host_definition, rle, sizes, flat, device):
    s = _marshal.RleSet("rle_convex_hull_host" if host_definition else "rle_convex_hull", rle, sizes, device, host_definition)
    hull_offs, xy, areas2, obb = _hull_flat(host_definition, s.space, s.counts, s.offs, *s.sides())
    if flat:
        return hull_offs, xy, areas2, obb
    o = s.space.host(hull_offs)
    return [xy[int(o[k]):int(o[k + 1])] for k in range(len(o) - 1)], areas2, obb


def rle_convex_hull(rle, sizes=None, flat=False, device=None):
    """The convex hull and the minimum-area oriented box of every mask of an RLE set, on the GPU from the runs
    (``mrcnn_rle_convex_hull``).  ``rle`` as rle_measure takes it; a pair of CUDA tensors gives tensors.  The hull of a mask is the
    hull of its set pixels' squares: a ring of integer pixel corners (x, y), strictly convex, clockwise on screen, starting at its
    smallest vertex by x then y; an empty mask has none.  flat=True returns (hull_offsets (n + 1), xy (V, 2), areas2 (n), obb (n, 8)),
    RLE k owning xy[hull_offsets[k]:hull_offsets[k + 1]], and nothing leaves the device; flat=False returns (hulls, areas2, obb) with
    one (m_k, 2) array per RLE (the offsets are read back).  areas2 is twice the hull's area.  obb is [e, dx, dy, dmin, dmax, cmin,
    cmax, 0]: the hull edge e, of vector (dx, dy), whose rectangle is smallest, and the extremes of d = dx*X + dy*Y and c = dx*Y -
    dy*X over the hull; the point (d, c) is ((d*dx - c*dy) / L2, (d*dy + c*dx) / L2) with L2 = dx^2 + dy^2; [-1, 0, ...] for an empty
    mask.  rle_region_props makes corners, centre, size and angle from it."""
    return _rle_convex_hull(False, rle, sizes, flat, device)


def rle_convex_hull_host(rle, sizes=None, flat=False):
    """The definition of rle_convex_hull: the sequential host code (``mrcnn_rle_convex_hull_host``), no GPU; numpy out."""
    return _rle_convex_hull(True, rle, sizes, flat, None)


REGION_PROPS = ("area", "centroid", "orientation", "major_axis", "minor_axis", "eccentricity", "perimeter", "compactness", "hull_area", "solidity",
                "extent", "obb_corners", "obb_center", "obb_size", "obb_angle")


def region_props_of(measures, hull_offsets, xy, areas2, obb):
    """The fields of rle_region_props from the integer tables (host arrays), computed with Python ints where 64 bits do not suffice."""
    import math
    n = int(len(measures))
    out = {"area": np.zeros(n, np.int64), "centroid": np.full((n, 2), np.nan), "orientation": np.full(n, np.nan), "major_axis": np.full(n, np.nan),
           "minor_axis": np.full(n, np.nan), "eccentricity": np.full(n, np.nan), "perimeter": np.zeros(n, np.int64), "compactness": np.full(n, np.nan),
           "hull_area": np.zeros(n), "solidity": np.full(n, np.nan), "extent": np.full(n, np.nan), "obb_corners": np.full((n, 4, 2), np.nan),
           "obb_center": np.full((n, 2), np.nan), "obb_size": np.full((n, 2), np.nan), "obb_angle": np.full(n, np.nan)}
    for k in range(n):
        s1, sx, sy, sxx, sxy, syy, per = (int(v) for v in measures[k])
        out["area"][k], out["perimeter"][k] = s1, per
        if s1 == 0:
            continue
        out["centroid"][k] = (sx / s1 + 0.5, sy / s1 + 0.5)
        c20 = (s1 * sxx - sx * sx) / (s1 * s1) + 1.0 / 12.0          # exact integers, one rounding each
        c02 = (s1 * syy - sy * sy) / (s1 * s1) + 1.0 / 12.0
        c11 = (s1 * sxy - sx * sy) / (s1 * s1)
        mean, dev = (c20 + c02) / 2.0, math.hypot((c20 - c02) / 2.0, c11)
        l1, l2 = mean + dev, max(mean - dev, 0.0)
        out["major_axis"][k], out["minor_axis"][k] = 4.0 * math.sqrt(l1), 4.0 * math.sqrt(l2)
        out["orientation"][k] = 0.5 * math.atan2(2.0 * c11, c20 - c02)
        out["eccentricity"][k] = math.sqrt(max(0.0, 1.0 - l2 / l1))
        out["compactness"][k] = 4.0 * math.pi * s1 / (per * per)
        a2 = int(areas2[k])
        out["hull_area"][k], out["solidity"][k] = a2 / 2, 2 * s1 / a2
        v = xy[int(hull_offsets[k]):int(hull_offsets[k + 1])]
        out["extent"][k] = s1 / ((int(v[:, 0].max()) - int(v[:, 0].min())) * (int(v[:, 1].max()) - int(v[:, 1].min())))
        _, dx, dy, dmin, dmax, cmin, cmax, _ = (int(t) for t in obb[k])
        L2 = dx * dx + dy * dy
        corners = [((d * dx - c * dy) / L2, (d * dy + c * dx) / L2) for d, c in ((dmin, cmin), (dmax, cmin), (dmax, cmax), (dmin, cmax))]
        out["obb_corners"][k] = corners
        out["obb_center"][k] = np.mean(np.asarray(corners), axis=0)
        out["obb_size"][k] = ((dmax - dmin) / math.sqrt(L2), (cmax - cmin) / math.sqrt(L2))
        out["obb_angle"][k] = math.atan2(dy, dx)
    return out


def _rle_region_props(host_definition, rle, sizes, device):
    s = _marshal.RleSet("rle_region_props_host" if host_definition else "rle_region_props", rle, sizes, device, host_definition)
    measures = _measure_flat(host_definition, s.space, s.counts, s.offs, *s.sides())
    tables = _hull_flat(host_definition, s.space, s.counts, s.offs, *s.sides())
    return region_props_of(s.space.host(measures), *(s.space.host(t) for t in tables))


def rle_region_props(rle, sizes=None, device=None):
    """The shape of every mask of an RLE set as skimage.regionprops and cv2.minAreaRect would give it, measured on the GPU from the runs
    (rle_measure and rle_convex_hull; only the small tables — n x 7, n x 8 and the hulls' vertices — are read back).  ``rle`` as
    rle_measure takes it.  Returns a dictionary of numpy arrays with one
    entry per RLE (k = b * slots + i for rows), coordinates in the tracer's corner frame (pixel (x, y) is [x, x+1] x [y, y+1], y down):
      area          S1                                   perimeter    the unit edges of the mask's outline (int64 both)
      centroid      (Sx / S1 + 1/2, Sy / S1 + 1/2)
      covariance    the pixel centres' (c20, c11, c02) = central second moments / S1, plus 1/12 on the diagonal for the uniform squares
      major_axis    4 * sqrt(l1)      minor_axis  4 * sqrt(l2)   of the covariance's eigenvalues l1 >= l2
      orientation   1/2 * atan2(2 * c11, c20 - c02), from +x towards +y      eccentricity  sqrt(1 - l2 / l1)
      compactness   4 * pi * S1 / perimeter^2
      hull_area     areas2 / 2        solidity    2 * S1 / areas2           extent  S1 / (the tight box's w * h)
      obb_corners   (4, 2): the points (dmin, cmin), (dmax, cmin), (dmax, cmax), (dmin, cmax) of the chosen edge's frame, clockwise on screen
      obb_center    their mean        obb_size    (D, C) / sqrt(L2): along and across the edge      obb_angle  atan2(dy, dx) of the edge
    An empty mask has area, perimeter and hull_area 0 and NaN elsewhere.  The central moments (S1 * Sxx - Sx^2) are taken in Python
    ints: they do not fit 64 bits."""
    return _rle_region_props(False, rle, sizes, device)


def rle_region_props_host(rle, sizes=None):
    """rle_region_props from the sequential host definitions (``mrcnn_rle_measure_host``, ``mrcnn_rle_convex_hull_host``), no GPU."""
    return _rle_region_props(True, rle, sizes, None)
