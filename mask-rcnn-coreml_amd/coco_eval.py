"""COCO scoring: the twelve numbers ``coco_dataset.evaluate_results`` prints at the end of the reference's ``maskrcnn evaluate``
(``Sources/maskrcnn/Python/COCOEval/task.py:93-98``), computed from the results ``coco_results.coco_results`` writes.

The procedure is COCO's published one (COCOeval: evaluate -> accumulate -> summarize).  Its hot half runs on the GPU through the C
ABI: the IoU of every detection with every ground truth of its image straight from the run lengths (``mrcnn_rle_iou``, or
``mrcnn_box_iou_xywh`` for ``bbox``) and the greedy matching for every (image, category, area range, threshold)
(``mrcnn_coco_match``), and COCOeval's accumulate (``mrcnn_coco_accumulate`` through ``accumulate_device``).  The host sorts each image's
detections, builds the group tables and runs ``summarize``; ``accumulate`` in numpy stays the definition of the device entry and the path
of a host without a device.  ``accumulate``, ``summarize`` and ``COCOGroundTruth`` need no GPU.  One deliberate difference to pycocotools: a detection counts as matched when it is matched, not
when the id of its ground truth is > 0.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .coco_results import rle_from_string

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ["all", "small", "medium", "large"]


def rle_from_polygons(polygons: Sequence[Sequence[float]], h: int, w: int) -> np.ndarray:
    """COCO polygons ([x0, y0, x1, y1, ...] each) of one annotation -> the run lengths of their union (mrcnn_rle_from_polygons)."""
    polys = [np.asarray(p, dtype=np.float64).reshape(-1) for p in polygons]
    for p in polys:
        if p.size % 2:
            raise ValueError("rle_from_polygons: a polygon is a flat list of x, y pairs")
    xy = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros(0), dtype=np.float64)
    offs = np.zeros(len(polys) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([p.size // 2 for p in polys])
    n = C.c_int64(0)
    L = _lib.lib()
    _lib.check(L.mrcnn_rle_from_polygons(xy.ctypes.data, offs.ctypes.data, len(polys), int(h), int(w), None, 0, C.byref(n)))
    out = np.empty(n.value, dtype=np.uint32)
    _lib.check(L.mrcnn_rle_from_polygons(xy.ctypes.data, offs.ctypes.data, len(polys), int(h), int(w), out.ctypes.data, out.size, C.byref(n)))
    return out


LDS_TOGGLES = 4096     # MRCNN_POLY_LDS_TOGGLES: an annotation whose outlines cross more pixel-column centres is sorted in global memory


def rle_from_polygons_batch(annotations_polygons, sizes, device=None):
    """The polygons of many annotations -> one ragged RLE set, encoded on the GPU in one call (mrcnn_rle_from_polygons_batch):
    annotations_polygons[k] = the COCO polygons of annotation k, sizes[k] = (h, w) of its image.  Returns (counts, run_offsets, areas,
    bboxes_xywh): RLE k = counts[run_offsets[k]:run_offsets[k + 1]], word for word what ``rle_from_polygons`` gives.  device=None:
    numpy arrays (uint32, int64, uint32, int32 (n, 4)); a torch device: tensors that stay there (int32, int64, int32, int32)."""
    polys, ann_offs = [], np.zeros(len(annotations_polygons) + 1, dtype=np.int64)
    for k, ann in enumerate(annotations_polygons):
        for p in ann:
            p = np.asarray(p, dtype=np.float64).reshape(-1)
            if p.size % 2:
                raise ValueError("rle_from_polygons_batch: a polygon is a flat list of x, y pairs")
            polys.append(p)
        ann_offs[k + 1] = len(polys)
    if len(sizes) != len(annotations_polygons):
        raise ValueError("rle_from_polygons_batch: one (h, w) per annotation")
    xy = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros(0), dtype=np.float64)
    offs = np.zeros(len(polys) + 1, dtype=np.int64)
    if polys:
        offs[1:] = np.cumsum([p.size // 2 for p in polys])
    n = len(annotations_polygons)
    hs = np.array([int(s[0]) for s in sizes], dtype=np.int32)
    ws = np.array([int(s[1]) for s in sizes], dtype=np.int32)
    L = _lib.lib()
    if device is None:
        ro = np.zeros(n + 1, dtype=np.int64)
        areas = np.zeros(n, dtype=np.uint32)
        boxes = np.zeros((n, 4), dtype=np.int32)
        ptr = lambda a: a.ctypes.data
        new = lambda c: np.empty(max(1, c), dtype=np.uint32)
        space, last = _lib.HOST, lambda: int(ro[n])
    else:
        import torch
        ro = torch.zeros(n + 1, dtype=torch.int64, device=device)
        areas = torch.zeros(n, dtype=torch.int32, device=device)
        boxes = torch.zeros((n, 4), dtype=torch.int32, device=device)
        ptr = lambda a: a.data_ptr()
        new = lambda c: torch.empty(max(1, c), dtype=torch.int32, device=device)
        space, last = _lib.DEVICE, lambda: int(ro[n].item())

    def call(capacity):
        counts = new(capacity)
        st = L.mrcnn_rle_from_polygons_batch(xy.ctypes.data, offs.ctypes.data, ann_offs.ctypes.data, n, hs.ctypes.data, ws.ctypes.data, space,
                                             ptr(counts), capacity, ptr(ro), ptr(areas), ptr(boxes))
        return st, counts
    capacity = 256 * n + 1024                                    # a guess; the call names what it needs
    st, counts = call(capacity)
    if st == 4 and last() > capacity:
        st, counts = call(last())
    _lib.check(st)
    return counts[:last()], ro, areas, boxes


def segmentation_to_counts(seg, h: int, w: int) -> np.ndarray:
    """Any of COCO's three segmentation forms -> uint32 run lengths on the h x w plane."""
    if isinstance(seg, dict):
        sh, sw = (int(v) for v in seg["size"])
        if (sh, sw) != (int(h), int(w)):
            raise ValueError(f"segmentation of size {sh}x{sw} on an image of {h}x{w}")
        c = seg["counts"]
        c = rle_from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.uint32)
    else:
        c = rle_from_polygons(seg, h, w)
    if int(c.astype(np.int64).sum()) != int(h) * int(w):
        raise ValueError(f"segmentation sums to {int(c.astype(np.int64).sum())} pixels, the image has {int(h) * int(w)}")
    return np.ascontiguousarray(c, dtype=np.uint32)


def _area(counts: np.ndarray) -> int:
    return int(counts[1::2].astype(np.int64).sum())


class COCOGroundTruth:
    """A COCO annotation file for scoring: ``images`` (id -> (h, w)), ``categories`` (sorted ids) and ``annotations`` in file order,
    each with image_id, category_id, iscrowd, area, bbox and — decoded on first use — its mask as run lengths."""

    def __init__(self, path_or_dict):
        if isinstance(path_or_dict, dict):
            d = path_or_dict
        else:
            with open(path_or_dict) as f:
                d = json.load(f)
        self.images: Dict = {im["id"]: (int(im["height"]), int(im["width"])) for im in d.get("images", [])}
        self.cat_ids: List = sorted(c["id"] for c in d.get("categories", []))
        self.annotations: List[dict] = []
        for a in d.get("annotations", []):
            self.annotations.append({"id": a.get("id"), "image_id": a["image_id"], "category_id": a["category_id"],
                                     "iscrowd": int(a.get("iscrowd", 0)), "area": a.get("area"), "bbox": a.get("bbox"),
                                     "segmentation": a.get("segmentation")})
        self.by_image: Dict = {}
        for a in self.annotations:
            self.by_image.setdefault(a["image_id"], []).append(a)

    def img_ids(self) -> List:
        return sorted(self.images)

    def counts(self, ann: dict) -> np.ndarray:
        if "_counts" not in ann:
            h, w = self.images[ann["image_id"]]
            ann["_counts"] = segmentation_to_counts(ann["segmentation"], h, w)
        return ann["_counts"]

    def area(self, ann: dict) -> float:
        if ann["area"] is not None:
            return float(ann["area"])
        if "_area" in ann:                                       # set pixels counted on the device (to_device)
            return ann["_area"]
        return float(_area(self.counts(ann)))

    def to_device(self, device="cuda") -> "DeviceGroundTruth":
        """Every annotation encoded once and kept on `device` for scoring (``score(..., device_gt=...)``): polygon annotations in one
        call of mrcnn_rle_from_polygons_batch, RLE-form annotations (crowds) decoded on the host and spliced in.  The order is that of
        ``by_image``, so the ground truths of an image are one contiguous range."""
        import torch
        order, ranges = [], {}
        for image_id, anns in self.by_image.items():
            ranges[image_id] = (len(order), len(order) + len(anns))
            order += anns
        n = len(order)
        sizes = [self.images[a["image_id"]] for a in order]
        is_poly = [not isinstance(a["segmentation"], dict) for a in order]
        poly_idx = [k for k in range(n) if is_poly[k]]
        pc, po, pa, _ = rle_from_polygons_batch([order[k]["segmentation"] for k in poly_idx], [sizes[k] for k in poly_idx], device=device)
        po_h = po.cpu().numpy()
        pa_h = pa.cpu().numpy()
        lengths = np.zeros(n, dtype=np.int64)
        host = {}
        for j, k in enumerate(poly_idx):
            lengths[k] = po_h[j + 1] - po_h[j]
        for k in range(n):
            if not is_poly[k]:
                host[k] = segmentation_to_counts(order[k]["segmentation"], *sizes[k])
                lengths[k] = host[k].size
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum(lengths)
        if host:
            counts = torch.empty(max(1, int(offs[n])), dtype=torch.int32, device=device)
            areas_h = np.zeros(n, dtype=np.int64)
            j = 0                                                # polygon annotations between two RLE-form ones move as one slice
            k = 0
            while k < n:
                if is_poly[k]:
                    k1 = k
                    while k1 < n and is_poly[k1]:
                        k1 += 1
                    m = k1 - k
                    counts[int(offs[k]):int(offs[k1])] = pc[int(po_h[j]):int(po_h[j + m])]
                    areas_h[k:k1] = pa_h[j:j + m]
                    j += m
                    k = k1
                else:
                    counts[int(offs[k]):int(offs[k + 1])] = torch.from_numpy(host[k].view(np.int32)).to(device)
                    areas_h[k] = _area(host[k])
                    k += 1
        else:
            counts, areas_h = pc, pa_h.astype(np.int64)
        run_offsets = torch.from_numpy(offs).to(device)
        areas = torch.from_numpy(areas_h.astype(np.int32)).to(device)
        # every RLE sums to the pixels of its image
        if n:
            csum = torch.zeros(int(offs[n]) + 1, dtype=torch.int64, device=device)
            csum[1:] = torch.cumsum(counts[:int(offs[n])].to(torch.int64) & 0xFFFFFFFF, 0)
            sums = (csum[run_offsets[1:]] - csum[run_offsets[:-1]]).cpu().numpy()
            want = np.array([h * w for h, w in sizes], dtype=np.int64)
            bad = np.nonzero(sums != want)[0]
            if bad.size:
                k = int(bad[0])
                raise ValueError(f"segmentation sums to {int(sums[k])} pixels, the image has {int(want[k])}")
        for k, a in enumerate(order):
            if a["area"] is None:
                a["_area"] = float(areas_h[k])
        return DeviceGroundTruth(self, counts, run_offsets, areas, offs, {id(a): k for k, a in enumerate(order)}, ranges,
                                 np.array([a["iscrowd"] for a in order], dtype=np.uint8), sizes)


class DeviceGroundTruth:
    """The masks of a COCOGroundTruth as one RLE set resident on the device, in the layout mrcnn_rle_iou reads: ``counts`` (int32),
    ``run_offsets`` (int64, n + 1) and ``areas`` (int32) are device tensors; annotation ``a`` is RLE ``index[id(a)]``, the annotations of
    an image are the range ``image_range[image_id]``; ``sizes[k]`` is the (h, w) of RLE k's image.  ``COCOGroundTruth.to_device`` makes
    one.  ``band(ratio)`` is the same set cut down to Boundary IoU's inner bands, made once per ratio where the runs lie."""

    def __init__(self, gt, counts, run_offsets, areas, host_offsets, index, image_range, iscrowd, sizes=None):
        self.gt, self.counts, self.run_offsets, self.areas = gt, counts, run_offsets, areas
        self.host_offsets, self.index, self.image_range, self.iscrowd = host_offsets, index, image_range, iscrowd
        self.n = len(index)
        self.sizes = sizes
        self._bands: Dict = {}

    def band(self, ratio: float = 0.02):
        """(counts, run_offsets, host_offsets) of the BOUNDARY set of every annotation (mrcnn_rle_morph on the resident runs), device
        tensors cached per ratio: every batch of a scoring run reads the same tensors."""
        key = float(ratio)
        if key not in self._bands:
            if self.sizes is None:
                raise ValueError("DeviceGroundTruth.band: the set was made without the sizes of its images")
            (c, o), _, _ = _band_set((self.counts, self.run_offsets[:self.n + 1]), self.sizes, key)
            self._bands[key] = (c, o, o.cpu().numpy())
        return self._bands[key]

    def gather(self, anns, band_ratio=None):
        """The RLEs of `anns` as a set of their own on the device (counts, run_offsets): when a filter breaks an image's range.
        band_ratio: their boundary bands at that ratio instead."""
        import torch
        src, host_offsets = (self.counts, self.host_offsets) if band_ratio is None else (self.band(band_ratio)[0], self.band(band_ratio)[2])
        ks = [self.index[id(a)] for a in anns]
        offs = np.zeros(len(ks) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([host_offsets[k + 1] - host_offsets[k] for k in ks])
        parts = [src[int(host_offsets[k]):int(host_offsets[k + 1])] for k in ks]
        counts = torch.cat(parts) if parts else torch.zeros(1, dtype=torch.int32, device=self.counts.device)
        return counts, torch.from_numpy(offs).to(self.counts.device)


# ------------------------------------------------------------------------------------------------------------------------------
# device half: IoU blocks and matching for one set of detections (host arrays, or a batch resident on the device)
# ------------------------------------------------------------------------------------------------------------------------------
class DeviceDetections:
    """The detections of a batch of images as they sit on the device behind ``mrcnn_masks_rle_source``: counts (cuda int32 tensor),
    run_offsets (cuda int64 tensor, B * rows + 1), and det_src / sizes / image_ids to name the rows.  ``device_detections`` makes one."""

    def __init__(self, image_ids, sizes, rows, counts, run_offsets, records):
        self.image_ids, self.sizes, self.rows = list(image_ids), list(sizes), int(rows)
        self.counts, self.run_offsets, self.records = counts, run_offsets, records
        self._bands: Dict = {}

    def band(self, ratio: float = 0.02):
        """(counts, run_offsets) of the BOUNDARY set of every row (mrcnn_rle_morph where the runs lie), cached per ratio."""
        key = float(ratio)
        if key not in self._bands:
            n = len(self.image_ids) * self.rows
            self._bands[key] = _band_set((self.counts, self.run_offsets[:n + 1]), [s for s in self.sizes for _ in range(self.rows)], key)[0]
        return self._bands[key]


def device_detections(image_ids, detections, masks, sizes, model_h: int, model_w: int, threshold: float = 0.5, class_to_category=None,
                      score_threshold: float = 0.0) -> DeviceDetections:
    """predict_images' device tensors -> DeviceDetections: the run lengths stay on the device; only the detection rows, the areas and
    the run offsets come to the host.  records = the COCO result records of coco_results.coco_results without ``segmentation``
    (``area`` and ``_row`` = (image of the batch, row) instead)."""
    import torch
    det, m = detections, masks
    B, rows = int(det.shape[0]), int(det.shape[1])
    hs = np.array([int(s[0]) for s in sizes], dtype=np.int32)
    ws = np.array([int(s[1]) for s in sizes], dtype=np.int32)
    n = B * rows
    det_src = torch.empty_like(det)
    areas = torch.empty((B, rows), dtype=torch.int32, device=det.device)
    offs = torch.empty(n + 1, dtype=torch.int64, device=det.device)
    L = _lib.lib()

    def call(capacity):
        counts = torch.empty(max(1, capacity), dtype=torch.int32, device=det.device)
        st = L.mrcnn_masks_rle_source(det.data_ptr(), m.data_ptr(), B, rows, int(m.shape[2]), hs.ctypes.data, ws.ctypes.data, model_h, model_w,
                                      C.c_float(threshold), _lib.DEVICE, det_src.data_ptr(), counts.data_ptr(), capacity, offs.data_ptr(),
                                      areas.data_ptr(), None)
        return st, counts
    capacity = int(rows * (2 * ws.astype(np.int64) + 2).sum())
    st, counts = call(capacity)
    need = int(offs[n].item())
    if st == 4 and need > capacity:
        st, counts = call(need)
    _lib.check(st)
    src = det_src.cpu().numpy()
    ar = areas.cpu().numpy()
    records = []
    for b, image_id in enumerate(image_ids):
        h, w = int(hs[b]), int(ws[b])
        for i in range(rows):
            r = src[b, i]
            score = float(r[5])
            if not score > score_threshold:
                continue
            y1 = int(np.rint(float(r[0]) * (h - 1))); x1 = int(np.rint(float(r[1]) * (w - 1)))
            y2 = int(np.rint(float(r[2]) * (h - 1) + 1.0)); x2 = int(np.rint(float(r[3]) * (w - 1) + 1.0))
            cls = int(r[4])
            records.append({"image_id": image_id, "category_id": int(class_to_category[cls]) if class_to_category is not None else cls,
                            "bbox": [float(x1), float(y1), float(x2 - x1), float(y2 - y1)], "score": score, "area": float(ar[b, i]),
                            "_row": (b, i)})
    return DeviceDetections(image_ids, [(int(a), int(b)) for a, b in zip(hs, ws)], rows, counts, offs, records)


def _band_set(pair, sizes, ratio: float, host_definition: bool = False):
    """detection.rle_morph(_host)(..., "boundary") on a flat (counts, run_offsets) pair with one (h, w) per RLE and Boundary IoU's radius
    for each: a pair of CUDA tensors stays on the device, numpy arrays go through the host definition when asked to."""
    from .detection import _rle_morph, boundary_radius
    radius: Dict = {}
    for s in sizes:
        if tuple(s) not in radius:
            radius[tuple(s)] = boundary_radius(int(s[0]), int(s[1]), ratio)
    if not len(sizes):
        return pair, None, None
    return _rle_morph(host_definition, pair, sizes, [radius[tuple(s)] for s in sizes], "boundary", None)


def _band_host(rles: List[np.ndarray], sizes, ratio: float) -> List[np.ndarray]:
    """the boundary bands of host RLEs, by the host definition (mrcnn_rle_morph_host)"""
    if not rles:
        return []
    (c, o), _, _ = _band_set(_concat_rles(rles), sizes, ratio, host_definition=True)
    return [c[int(o[k]):int(o[k + 1])] for k in range(len(rles))]


def _gt_bands(gt: "COCOGroundTruth", anns: List[dict], ratio: float) -> List[np.ndarray]:
    """the bands of ground-truth annotations on the host, cached per annotation and ratio"""
    todo = [a for a in anns if float(ratio) not in a.setdefault("_band", {})]
    todo = list({id(a): a for a in todo}.values())
    for a, b in zip(todo, _band_host([gt.counts(a) for a in todo], [gt.images[a["image_id"]] for a in todo], ratio)):
        a["_band"][float(ratio)] = b
    return [a["_band"][float(ratio)] for a in anns]


def _concat_rles(rles: List[np.ndarray]):
    offs = np.zeros(len(rles) + 1, dtype=np.int64)
    if rles:
        offs[1:] = np.cumsum([r.size for r in rles])
    counts = np.ascontiguousarray(np.concatenate(rles) if rles else np.zeros(0, np.uint32), dtype=np.uint32)
    return counts, offs


def _group_array(groups):
    arr = (_lib.IouGroup * max(1, len(groups)))()
    for k, g in enumerate(groups):
        arr[k].d0, arr[k].d1, arr[k].g0, arr[k].g1, arr[k].out_offset = g
    return arr


def _evaluate_set(gt: COCOGroundTruth, img_order: List, per_image: Dict, iou_type: str, max_det: int, device: Optional[DeviceDetections],
                  cat_set, area_rng, iou_thrs, resident: Optional["DeviceGroundTruth"] = None, boundary_ratio: float = 0.02):
    """IoU + matching for the images of one detection set.  per_image[image_id] = list of records (with ``_local`` = the row of the
    image's IoU block, ``area``, ``score``, ``category_id`` and — host sets — ``_counts``).  Returns {(image_id, category_id): eval}."""
    L = _lib.lib()
    A, T = len(area_rng), len(iou_thrs)
    on_device = device is not None
    band = iou_type == "boundary"                                # the mask IoU, then the bands' IoU and the smaller of the two
    if band:
        iou_type = "segm"
    if resident is not None and (iou_type != "segm" or resident.gt is not gt):
        resident = None                                          # boxes are host tables; another file's set is not this one's
    iou_dev = on_device or resident is not None                  # where the IoU blocks live
    in_place = resident is not None                              # the images' ranges of the resident set, unless a filter breaks one
    imgs = [i for i in img_order if i in per_image]
    # --- the two sets and the IoU groups -----------------------------------------------------------------------------------------
    g_anns, groups, blocks = [], [], {}
    d_rles, d_sizes, d_boxes, out_at, d_at = [], [], [], 0, 0
    for image_id in imgs:
        recs = per_image[image_id]
        ganns = [a for a in gt.by_image.get(image_id, []) if a["category_id"] in cat_set]
        if on_device:
            b = device.image_ids.index(image_id)
            d0, nd = b * device.rows, device.rows
        else:
            d0, nd = d_at, len(recs)
            d_at += nd
            if iou_type == "segm":
                d_rles += [r["_counts"] for r in recs]
                d_sizes += [gt.images[image_id]] * nd
        if iou_type == "bbox":
            if on_device:
                rows = np.zeros((device.rows, 4), np.float64)
                for r in recs:
                    rows[r["_local"]] = r["bbox"]
                d_boxes.append(rows)
            else:
                d_boxes.append(np.array([r["bbox"] for r in recs], dtype=np.float64).reshape(-1, 4))
        g0 = len(g_anns)
        g_anns += ganns
        if in_place and ganns:
            r0, r1 = resident.image_range[image_id]
            in_place = r1 - r0 == len(ganns)
            g0 = r0
        groups.append((d0, d0 + nd, g0, g0 + len(ganns), out_at))
        blocks[image_id] = (out_at, len(ganns), ganns)
        out_at += nd * len(ganns)
    n_pairs, n_g = out_at, len(g_anns)
    crowd = np.array([a["iscrowd"] for a in g_anns], dtype=np.uint8)
    if resident is not None and not in_place:                    # the gather fallback: the groups name the gathered set
        at = 0
        for k, (image_id, g) in enumerate(zip(imgs, groups)):
            ng = g[3] - g[2]
            groups[k] = (g[0], g[1], at, at + ng, g[4])
            at += ng
    g_lo = 0
    if resident is not None and in_place:                        # only the stretch of the resident set this batch's images span is named
        used = [g for g in groups if g[3] > g[2]]
        g_lo, g_hi = (min(g[2] for g in used), max(g[3] for g in used)) if used else (0, 0)
        groups = [(g[0], g[1], g[2] - g_lo, g[3] - g_lo, g[4]) if g[3] > g[2] else (g[0], g[1], 0, 0, g[4]) for g in groups]
    garr = _group_array(groups)
    if iou_dev:
        import torch
        dev_of = device.counts.device if on_device else resident.counts.device
        iou = torch.zeros(max(1, n_pairs), dtype=torch.float64, device=dev_of)
        iou_ptr, space = iou.data_ptr(), _lib.DEVICE
    else:
        iou = np.zeros(max(1, n_pairs), dtype=np.float64)
        iou_ptr, space = iou.ctypes.data, _lib.HOST
    if n_pairs:
        if iou_type == "segm" and resident is not None:
            # the ground truth never leaves the device: its resident buffers, or a gather of them on the device
            if in_place:
                gc, go, n_g = resident.counts, resident.run_offsets[g_lo:g_hi + 1], g_hi - g_lo      # (the offsets index the whole counts)
                crowd = np.ascontiguousarray(resident.iscrowd[g_lo:g_hi])
            else:
                gc, go = resident.gather(g_anns)
            if on_device:
                dc, do, n_d = device.counts, device.run_offsets, len(device.image_ids) * device.rows
            else:
                d_counts, d_offs = _concat_rles(d_rles)
                dc = torch.from_numpy(d_counts.view(np.int32)).to(dev_of) if d_counts.size else torch.zeros(1, dtype=torch.int32, device=dev_of)
                do, n_d = torch.from_numpy(d_offs).to(dev_of), len(d_rles)
            _lib.check(L.mrcnn_rle_iou(dc.data_ptr(), do.data_ptr(), n_d, gc.data_ptr(), go.data_ptr(), n_g, crowd.ctypes.data, garr, len(groups),
                                       space, None, iou_ptr, n_pairs))
            if band:                                             # the same groups over the two band sets, made where the runs lie
                if in_place:
                    gc, go = resident.band(boundary_ratio)[0], resident.band(boundary_ratio)[1][g_lo:g_hi + 1]
                else:
                    gc, go = resident.gather(g_anns, boundary_ratio)
                if on_device:
                    dc, do = device.band(boundary_ratio)
                else:
                    d_counts, d_offs = _concat_rles(_band_host(d_rles, d_sizes, boundary_ratio))
                    dc = torch.from_numpy(d_counts.view(np.int32)).to(dev_of) if d_counts.size else torch.zeros(1, dtype=torch.int32, device=dev_of)
                    do = torch.from_numpy(d_offs).to(dev_of)
                iou_b = torch.zeros_like(iou)
                _lib.check(L.mrcnn_rle_iou(dc.data_ptr(), do.data_ptr(), n_d, gc.data_ptr(), go.data_ptr(), n_g, crowd.ctypes.data, garr, len(groups),
                                           space, None, iou_b.data_ptr(), n_pairs))
                torch.minimum(iou, iou_b, out=iou)
        elif iou_type == "segm":
            g_counts, g_offs = _concat_rles([gt.counts(a) for a in g_anns])
            if on_device:
                gc = torch.from_numpy(g_counts.view(np.int32)).to(device.counts.device)
                go = torch.from_numpy(g_offs).to(device.counts.device)
                n_d = len(device.image_ids) * device.rows
                _lib.check(L.mrcnn_rle_iou(device.counts.data_ptr(), device.run_offsets.data_ptr(), n_d, gc.data_ptr(), go.data_ptr(), n_g,
                                           crowd.ctypes.data, garr, len(groups), space, None, iou_ptr, n_pairs))
                if band:                                         # the detections' bands where their runs lie, the ground truth's uploaded
                    g_counts, g_offs = _concat_rles(_gt_bands(gt, g_anns, boundary_ratio))
                    gc = torch.from_numpy(g_counts.view(np.int32)).to(device.counts.device)
                    go = torch.from_numpy(g_offs).to(device.counts.device)
                    dc, do = device.band(boundary_ratio)
                    iou_b = torch.zeros_like(iou)
                    _lib.check(L.mrcnn_rle_iou(dc.data_ptr(), do.data_ptr(), n_d, gc.data_ptr(), go.data_ptr(), n_g, crowd.ctypes.data, garr,
                                               len(groups), space, None, iou_b.data_ptr(), n_pairs))
                    torch.minimum(iou, iou_b, out=iou)
            else:
                d_counts, d_offs = _concat_rles(d_rles)
                _lib.check(L.mrcnn_rle_iou(d_counts.ctypes.data, d_offs.ctypes.data, len(d_rles), g_counts.ctypes.data, g_offs.ctypes.data, n_g,
                                           crowd.ctypes.data, garr, len(groups), space, None, iou_ptr, n_pairs))
                if band:                                         # host sets: the host definition and the host memspace of mrcnn_rle_iou
                    d_counts, d_offs = _concat_rles(_band_host(d_rles, d_sizes, boundary_ratio))
                    g_counts, g_offs = _concat_rles(_gt_bands(gt, g_anns, boundary_ratio))
                    iou_b = np.zeros_like(iou)
                    _lib.check(L.mrcnn_rle_iou(d_counts.ctypes.data, d_offs.ctypes.data, len(d_rles), g_counts.ctypes.data, g_offs.ctypes.data, n_g,
                                               crowd.ctypes.data, garr, len(groups), space, None, iou_b.ctypes.data, n_pairs))
                    np.minimum(iou, iou_b, out=iou)
        else:
            db = np.ascontiguousarray(np.concatenate(d_boxes) if d_boxes else np.zeros((0, 4)), dtype=np.float64)
            gb = np.ascontiguousarray(np.array([a["bbox"] for a in g_anns], dtype=np.float64).reshape(-1, 4))
            if on_device:
                # boxes are small host tables: the device rows are addressed by (image of the batch, row) like the RLEs
                full = np.zeros((len(device.image_ids) * device.rows, 4), np.float64)
                for image_id, rows in zip(imgs, d_boxes):
                    b = device.image_ids.index(image_id)
                    full[b * device.rows:(b + 1) * device.rows] = rows
                dbt, gbt = torch.from_numpy(full).to(iou.device), torch.from_numpy(gb).to(iou.device)
                _lib.check(L.mrcnn_box_iou_xywh(dbt.data_ptr(), full.shape[0], gbt.data_ptr(), n_g, crowd.ctypes.data, garr, len(groups), space,
                                                iou_ptr, n_pairs))
            else:
                _lib.check(L.mrcnn_box_iou_xywh(db.ctypes.data, db.shape[0], gb.ctypes.data, n_g, crowd.ctypes.data, garr, len(groups), space,
                                                iou_ptr, n_pairs))
    # --- the match groups: (image, category) --------------------------------------------------------------------------------------
    mgroups, keys = [], []
    dt_idx, dt_area, gt_idx, gt_area, gt_crowd = [], [], [], [], []
    for image_id in imgs:
        off, ng_img, ganns = blocks[image_id]
        recs = per_image[image_id]
        cats = sorted(set(r["category_id"] for r in recs) | set(a["category_id"] for a in ganns))
        for cat in cats:
            dts = [r for r in recs if r["category_id"] == cat]
            order = np.argsort([-r["score"] for r in dts], kind="mergesort")[:max_det]
            dts = [dts[i] for i in order]
            gcols = [j for j, a in enumerate(ganns) if a["category_id"] == cat]
            d0, g0 = len(dt_idx), len(gt_idx)
            dt_idx += [r["_local"] for r in dts]
            dt_area += [r["area"] for r in dts]
            gt_idx += gcols
            gt_area += [gt.area(ganns[j]) for j in gcols]
            gt_crowd += [ganns[j]["iscrowd"] for j in gcols]
            mgroups.append((off, ng_img, d0, len(dt_idx), g0, len(gt_idx)))
            keys.append((image_id, cat, dts, [ganns[j] for j in gcols]))
    out = {}
    if not mgroups:
        return out
    marr = (_lib.MatchGroup * len(mgroups))()
    for k, g in enumerate(mgroups):
        marr[k].iou_offset, marr[k].iou_stride, marr[k].dt0, marr[k].dt1, marr[k].gt0, marr[k].gt1 = g
    dt_idx_a = np.array(dt_idx, dtype=np.int32); dt_area_a = np.array(dt_area, dtype=np.float64)
    gt_idx_a = np.array(gt_idx, dtype=np.int32); gt_area_a = np.array(gt_area, dtype=np.float64); gt_crowd_a = np.array(gt_crowd, dtype=np.uint8)
    rng = np.ascontiguousarray(area_rng, dtype=np.float64); thr = np.ascontiguousarray(iou_thrs, dtype=np.float64)
    n_dt, n_gt = dt_idx_a.size, gt_idx_a.size
    dt_match = np.full(max(1, A * T * n_dt), -1, dtype=np.int32)
    dt_ignore = np.zeros(max(1, A * T * n_dt), dtype=np.uint8)
    if iou_dev:
        dm = torch.empty(max(1, A * T * n_dt), dtype=torch.int32, device=iou.device)
        di = torch.empty(max(1, A * T * n_dt), dtype=torch.uint8, device=iou.device)
        _lib.check(L.mrcnn_coco_match(iou_ptr, n_pairs, space, marr, len(mgroups), dt_idx_a.ctypes.data, dt_area_a.ctypes.data, n_dt, gt_idx_a.ctypes.data,
                                      gt_area_a.ctypes.data, gt_crowd_a.ctypes.data, n_gt, rng.ctypes.data, A, thr.ctypes.data, T, dm.data_ptr(),
                                      di.data_ptr(), None))
        dt_match, dt_ignore = dm.cpu().numpy(), di.cpu().numpy()
    else:
        _lib.check(L.mrcnn_coco_match(iou_ptr, n_pairs, space, marr, len(mgroups), dt_idx_a.ctypes.data, dt_area_a.ctypes.data, n_dt, gt_idx_a.ctypes.data,
                                      gt_area_a.ctypes.data, gt_crowd_a.ctypes.data, n_gt, rng.ctypes.data, A, thr.ctypes.data, T, dt_match.ctypes.data,
                                      dt_ignore.ctypes.data, None))
    for (image_id, cat, dts, gts), g in zip(keys, mgroups):
        d0, d1 = g[2], g[3]
        nd = d1 - d0
        m = dt_match[A * T * d0:A * T * d1].reshape(A, T, nd)
        ig = dt_ignore[A * T * d0:A * T * d1].reshape(A, T, nd)
        out[(image_id, cat)] = {"scores": np.array([r["score"] for r in dts], dtype=np.float64), "matched": m >= 0, "ignore": ig != 0,
                                "gt_ignore": gt_ignore_flags(gts, gt, area_rng)}
    return out


def gt_ignore_flags(gts: List[dict], gt: COCOGroundTruth, area_rng) -> np.ndarray:
    """(A, ng) bool: crowd, or area outside the range (COCOeval.evaluateImg's ``_ignore``)."""
    ar = np.array([gt.area(a) for a in gts], dtype=np.float64)
    crowd = np.array([bool(a["iscrowd"]) for a in gts], dtype=bool)
    rng = np.asarray(area_rng, dtype=np.float64)
    return crowd[None, :] | (ar[None, :] < rng[:, :1]) | (ar[None, :] > rng[:, 1:])


# ------------------------------------------------------------------------------------------------------------------------------
# host half: accumulate / summarize (numpy, no GPU)
# ------------------------------------------------------------------------------------------------------------------------------
def accumulate(evals: List[List[dict]], max_dets=(1, 10, 100), n_thrs: int = len(IOU_THRS), n_areas: int = len(AREA_RNG), rec_thrs=REC_THRS):
    """COCOeval.accumulate.  evals[k] = the per-image records of category k, in image order; a record holds ``scores`` (nd, descending),
    ``matched`` / ``ignore`` (A, T, nd) bool and ``gt_ignore`` (A, ng) bool.  Returns precision (T, R, K, A, M), recall (T, K, A, M)."""
    T, R, K, A, M = n_thrs, len(rec_thrs), len(evals), n_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, E in enumerate(evals):
        if not E:
            continue
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                scores = np.concatenate([e["scores"][:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["matched"][a][:, :max_det] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["ignore"][a][:, :max_det] for e in E], axis=1)[:, inds]
                gtig = np.concatenate([e["gt_ignore"][a] for e in E])
                npig = np.count_nonzero(gtig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(idx):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


ACC_CHUNK = 1024       # MRCNN_COCO_ACC_CHUNK: mrcnn_coco_accumulate sorts and scans a category in chunks of this many entries


def pack_evals(evals: List[List[dict]], max_dets=(1, 10, 100), n_thrs: int = len(IOU_THRS), n_areas: int = len(AREA_RNG)) -> dict:
    """The per-category lists of per-image records ``accumulate`` takes -> the flat tables of mrcnn_coco_accumulate: ``scores`` (n,
    float64), ``ranks`` (n, int32: the position in the record), ``matched`` / ``ignore`` (A, T, n) uint8, ``cat_offsets`` (K + 1, int64) and
    ``npig`` (K, A) int64.  The entries are accumulate's concatenation for the largest of max_dets: category after category, record after
    record, each record cut to that many entries."""
    K, A, T, cap = len(evals), int(n_areas), int(n_thrs), int(max(max_dets))
    recs = [e for E in evals for e in E]
    rec_bounds = np.zeros(K + 1, dtype=np.int64)
    rec_bounds[1:] = np.cumsum(np.fromiter((len(E) for E in evals), dtype=np.int64, count=K))
    lens = np.fromiter((len(e["scores"]) for e in recs), dtype=np.int64, count=len(recs))
    ngs = np.fromiter((np.shape(e["gt_ignore"])[1] for e in recs), dtype=np.int64, count=len(recs))
    if recs:
        scores = np.concatenate([e["scores"] for e in recs]).astype(np.float64, copy=False)
        matched = np.concatenate([e["matched"] for e in recs], axis=2)
        ignore = np.concatenate([e["ignore"] for e in recs], axis=2)
        gt_ignore = np.concatenate([e["gt_ignore"] for e in recs], axis=1)
    else:
        scores, matched, ignore, gt_ignore = np.zeros(0), np.zeros((A, T, 0), bool), np.zeros((A, T, 0), bool), np.zeros((A, 0), bool)
    n = int(lens.sum())
    if matched.shape != (A, T, n) or ignore.shape != (A, T, n) or gt_ignore.shape[0] != A or scores.shape != (n,):
        raise ValueError(f"pack_evals: records of {n} entries with flags of shape {matched.shape} / {ignore.shape} and ground-truth flags "
                         f"{gt_ignore.shape}: expected ({A}, {T}, {n}) and ({A}, ng)")
    ranks = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    if n and int(lens.max()) > cap:                              # accumulate's [:max_det] for the largest max_det
        keep = ranks < cap
        scores, ranks, matched, ignore = scores[keep], ranks[keep], matched[:, :, keep], ignore[:, :, keep]
        lens = np.minimum(lens, cap)
    ends = np.zeros(len(recs) + 1, dtype=np.int64)
    ends[1:] = np.cumsum(lens)
    g_ends = np.zeros(len(recs) + 1, dtype=np.int64)
    g_ends[1:] = np.cumsum(ngs)
    found = np.zeros((A, gt_ignore.shape[1] + 1), dtype=np.int64)
    found[:, 1:] = np.cumsum(gt_ignore == 0, axis=1)
    g_bounds = g_ends[rec_bounds]
    npig = (found[:, g_bounds[1:]] - found[:, g_bounds[:-1]]).T
    return {"scores": np.ascontiguousarray(scores, dtype=np.float64), "ranks": np.ascontiguousarray(ranks, dtype=np.int32),
            "matched": np.ascontiguousarray(matched != 0, dtype=np.uint8), "ignore": np.ascontiguousarray(ignore != 0, dtype=np.uint8),
            "cat_offsets": np.ascontiguousarray(ends[rec_bounds]), "npig": np.ascontiguousarray(npig, dtype=np.int64)}


def accumulate_packed(packed: dict, max_dets=(1, 10, 100), rec_thrs=REC_THRS, device=None):
    """mrcnn_coco_accumulate over the tables of ``pack_evals``.  device=None: the tables stay numpy arrays and the library stages them;
    a torch device: they are uploaded as tensors and read in place.  Returns precision (T, R, K, A, M), recall (T, K, A, M) as numpy."""
    A, T, n = packed["matched"].shape
    K, M = packed["cat_offsets"].size - 1, len(max_dets)
    md = np.ascontiguousarray(max_dets, dtype=np.int32)
    thr = np.ascontiguousarray(rec_thrs, dtype=np.float64)
    R = thr.size
    L = _lib.lib()
    tables = [packed["scores"], packed["ranks"], packed["matched"], packed["ignore"]]
    if device is None:
        precision, recall = np.empty((T, R, K, A, M)), np.empty((T, K, A, M))
        ptr, space = (lambda a: a.ctypes.data), _lib.HOST
    else:
        import torch
        tables = [torch.from_numpy(a).to(device) for a in tables]
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=device)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=device)
        ptr, space = (lambda a: a.data_ptr()), _lib.DEVICE
    _lib.check(L.mrcnn_coco_accumulate(ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(tables[3]), n, packed["cat_offsets"].ctypes.data, K,
                                       packed["npig"].ctypes.data, A, T, md.ctypes.data, M, thr.ctypes.data, R, space, ptr(precision), ptr(recall)))
    if device is not None:
        precision, recall = precision.cpu().numpy(), recall.cpu().numpy()
    return precision, recall


def accumulate_device(evals: List[List[dict]], max_dets=(1, 10, 100), n_thrs: int = len(IOU_THRS), n_areas: int = len(AREA_RNG), rec_thrs=REC_THRS,
                      device="cuda"):
    """``accumulate`` on the GPU (mrcnn_coco_accumulate): the same arguments, the same two arrays bit for bit.  device: where the packed
    tables are uploaded as torch tensors, or None to hand the library host arrays."""
    return accumulate_packed(pack_evals(evals, max_dets, n_thrs, n_areas), max_dets, rec_thrs, device)


# What accumulate_on=None means.  The device entry has not been timed against numpy's accumulate on an MI355X yet (DESIGN.md §5
# "Scoring"; tools/coco_accumulate_ab.py takes the measurement), so the default stays with the definition; "device" is for the asking.
DEFAULT_ACCUMULATE_ON = "host"


def _accumulate_where(accumulate_on):
    """None: DEFAULT_ACCUMULATE_ON — and the host in any case when there is no device."""
    if accumulate_on is None:
        return "device" if DEFAULT_ACCUMULATE_ON == "device" and _lib.lib().mrcnn_device_count() > 0 else "host"
    if accumulate_on not in ("host", "device"):
        raise ValueError("accumulate_on must be None, 'host' or 'device'")
    return accumulate_on


def summarize(precision: np.ndarray, recall: np.ndarray, max_dets=(1, 10, 100), iou_thrs=IOU_THRS, area_lbl=AREA_LBL):
    """COCOeval.summarize: (stats (12,), the twelve lines)."""
    lines = []

    def one(ap, iou_thr=None, area="all", max_det=100):
        a, m = area_lbl.index(area), list(max_dets).index(max_det)
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == np.asarray(iou_thrs))[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        v = -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
        iou_str = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1]) if iou_thr is None else "{:0.2f}".format(iou_thr)
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_str, area, max_det, v))
        return v
    md = list(max_dets)
    stats = np.array([one(1, max_det=md[2]), one(1, .5, max_det=md[2]), one(1, .75, max_det=md[2]), one(1, area="small", max_det=md[2]),
                      one(1, area="medium", max_det=md[2]), one(1, area="large", max_det=md[2]), one(0, max_det=md[0]), one(0, max_det=md[1]),
                      one(0, max_det=md[2]), one(0, area="small", max_det=md[2]), one(0, area="medium", max_det=md[2]),
                      one(0, area="large", max_det=md[2])])
    return stats, lines


def _records(gt: COCOGroundTruth, results, iou_type: str, img_set, cat_set):
    """The results of the scored images and categories per image, each with its area (and its run lengths for ``segm`` and
    ``boundary``, whose areas are the MASK areas)."""
    per_image: Dict = {}
    for r in results:
        if r["image_id"] not in img_set or r["category_id"] not in cat_set:
            continue
        rec = {"image_id": r["image_id"], "category_id": r["category_id"], "score": float(r["score"])}
        if iou_type in ("segm", "boundary"):
            h, w = gt.images[r["image_id"]]
            rec["_counts"] = segmentation_to_counts(r["segmentation"], h, w)
            rec["area"] = float(_area(rec["_counts"]))
        else:
            rec["bbox"] = [float(v) for v in r["bbox"]]
            rec["area"] = rec["bbox"][2] * rec["bbox"][3]
        lst = per_image.setdefault(r["image_id"], [])
        rec["_local"] = len(lst)
        lst.append(rec)
    return per_image


def _finish(gt: COCOGroundTruth, ev: Dict, img_ids: List, cat_ids: List, max_dets, accumulate_on=None):
    where = _accumulate_where(accumulate_on)
    cat_set = set(cat_ids)
    for image_id in img_ids:                                  # images with ground truth and no detection at all still count their objects
        by_cat: Dict = {}
        for a in gt.by_image.get(image_id, []):
            if a["category_id"] in cat_set:
                by_cat.setdefault(a["category_id"], []).append(a)
        for cat, gts in by_cat.items():
            if (image_id, cat) not in ev:
                A, T = len(AREA_RNG), len(IOU_THRS)
                ev[(image_id, cat)] = {"scores": np.zeros(0), "matched": np.zeros((A, T, 0), bool), "ignore": np.zeros((A, T, 0), bool),
                                       "gt_ignore": gt_ignore_flags(gts, gt, AREA_RNG)}
    evals = [[ev[(i, c)] for i in img_ids if (i, c) in ev] for c in cat_ids]
    precision, recall = accumulate_device(evals, max_dets, device=None) if where == "device" else accumulate(evals, max_dets)
    stats, lines = summarize(precision, recall, max_dets)
    return {"stats": stats, "precision": precision, "recall": recall, "summary": lines, "img_ids": list(img_ids), "cat_ids": list(cat_ids)}


def score(gt: COCOGroundTruth, results, iou_type: str = "segm", img_ids=None, max_dets=(1, 10, 100), device_batches=None, device_gt=None,
          accumulate_on=None, boundary_ratio: float = 0.02) -> dict:
    """COCO's twelve numbers for `results` (the list coco_results.coco_results returns, or that list loaded from JSON) against `gt`.
    Returns ``stats`` (12, -1 where COCO prints -1), ``precision`` (T, R, K, A, M), ``recall`` (T, K, A, M) and ``summary`` (the twelve
    lines in COCOeval's wording).  img_ids: the images scored (default: all of the annotation file).
    device_batches: a list of DeviceDetections — the fast path: `results` may then be None; the run lengths of those batches are read
    on the device where mrcnn_masks_rle_source left them (see score_batch).
    device_gt: ``gt.to_device()`` — for ``segm`` the ground truth is then read where it is resident, for every batch, and no run length
    of it crosses to the device again; the numbers are the same.
    accumulate_on: "device" — COCOeval's accumulate through mrcnn_coco_accumulate, "host" — in numpy, None — DEFAULT_ACCUMULATE_ON; the
    arrays are identical either way.
    iou_type "boundary": Boundary AP (Cheng et al., CVPR 2021).  Per image r = detection.boundary_radius(h, w, boundary_ratio); the IoU
    of a pair is the smaller of its mask IoU and the IoU of the two inner bands of width r (mrcnn_rle_morph's BOUNDARY), the crowd
    rule applied in both; areas, matching, accumulate and summarize are those of ``segm``.  Device sets get their bands where the
    runs lie and the minimum is taken on the device; ``device_gt`` keeps its bands per ratio for every batch; host sets go through
    mrcnn_rle_morph_host, cached per annotation."""
    _accumulate_where(accumulate_on)
    if iou_type not in ("segm", "bbox", "boundary"):
        raise ValueError("iou_type must be 'segm', 'bbox' or 'boundary'")
    if not (np.isfinite(boundary_ratio) and boundary_ratio > 0):
        raise ValueError("boundary_ratio must be finite and > 0")
    if len(max_dets) != 3:
        raise ValueError("max_dets: three values, as COCO's summary reads them")
    img_ids = sorted(set(gt.img_ids() if img_ids is None else img_ids))
    cat_ids = list(gt.cat_ids)
    img_set, cat_set = set(img_ids), set(cat_ids)
    ev: Dict = {}
    if device_batches is not None:
        for batch in device_batches:
            per_image: Dict = {}
            for r in batch.records:
                if r["image_id"] in img_set and r["category_id"] in cat_set:
                    rec = dict(r)
                    rec["_local"] = r["_row"][1]
                    if iou_type == "bbox":
                        rec["area"] = r["bbox"][2] * r["bbox"][3]
                    per_image.setdefault(r["image_id"], []).append(rec)
            ev.update(_evaluate_set(gt, img_ids, per_image, iou_type, max_dets[-1], batch, cat_set, AREA_RNG, IOU_THRS, device_gt, boundary_ratio))
    else:
        per_image = _records(gt, results or [], iou_type, img_set, cat_set)
        ev.update(_evaluate_set(gt, img_ids, per_image, iou_type, max_dets[-1], None, cat_set, AREA_RNG, IOU_THRS, device_gt, boundary_ratio))
    return _finish(gt, ev, img_ids, cat_ids, max_dets, accumulate_on)


def score_batch(gt: COCOGroundTruth, batches: Sequence[DeviceDetections], iou_type: str = "segm", img_ids=None, max_dets=(1, 10, 100),
                device_gt=None, accumulate_on=None, boundary_ratio: float = 0.02) -> dict:
    """``score`` over detections that never left the device (device_detections): the same arrays as the path through strings.  With
    device_gt = ``gt.to_device()`` neither side of the mask IoU is uploaded per batch — nor, for "boundary", of the bands' IoU."""
    return score(gt, None, iou_type, img_ids, max_dets, device_batches=list(batches), device_gt=device_gt, accumulate_on=accumulate_on,
                 boundary_ratio=boundary_ratio)
