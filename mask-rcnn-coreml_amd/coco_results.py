"""COCO run-length encoded masks and the COCO results file (``segm`` / ``bbox`` detections) a scorer reads.

The scoring half of the reference's ``maskrcnn evaluate`` (``Sources/maskrcnn/Python/COCOEval/task.py:93-98``,
``coco_dataset.evaluate_results``) wants COCO-format results; the reference's own ``results.proto`` drops the masks.  Here the masks
arrive already run-length encoded from the GPU (``detection.masks_rle_source`` / ``mrcnn_masks_rle_source``); this module turns them
into COCO's compressed strings (``mrcnn_rle_to_string`` / ``mrcnn_rle_from_string``, host arithmetic of the C library) and into the
list of result records.  ``rle_decode`` / ``rle_encode`` are numpy helpers for consumers and tests.  No GPU involved, unless
``coco_results(segmentation="polygon")`` is asked to trace the rings itself.

An RLE here is ``{"size": [h, w], "counts": ...}`` as in pycocotools: pixels in column-major order, ``counts[0]`` the number of
leading zeros, then alternating run lengths of ones and zeros.  ``counts`` is a uint32 array (uncompressed) or a ``str`` (compressed).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib


def rle_to_string(counts) -> str:
    """Run lengths → COCO's compressed string."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    n = C.c_int64(0)
    buf = C.create_string_buffer(max(1, 7 * c.size))           # a 32-bit value (33 with the sign) takes at most 7 characters
    _lib.check(_lib.lib().mrcnn_rle_to_string(c.ctypes.data, c.size, buf, 7 * c.size, C.byref(n)))
    return buf.raw[:n.value].decode("ascii")


def rle_from_string(s) -> np.ndarray:
    """COCO's compressed string → run lengths (uint32)."""
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    n = C.c_int64(0)
    out = np.empty(max(1, len(b)), dtype=np.uint32)            # every count takes at least one character
    _lib.check(_lib.lib().mrcnn_rle_from_string(b, len(b), out.ctypes.data, len(b), C.byref(n)))
    return out[:n.value].copy()


def _counts(rle) -> np.ndarray:
    c = rle["counts"]
    return rle_from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.uint32)


def rle_decode(rle) -> np.ndarray:
    """RLE → the (h, w) uint8 {0,1} plane."""
    h, w = (int(v) for v in rle["size"])
    c = _counts(rle).astype(np.int64)
    if int(c.sum()) != h * w:
        raise ValueError(f"rle_decode: the counts sum to {int(c.sum())}, the plane has {h * w} pixels")
    bits = (np.arange(c.size) & 1).astype(np.uint8)
    return np.repeat(bits, c).reshape(w, h).T.copy()


def rle_encode(plane: np.ndarray) -> Dict:
    """(h, w) plane (non-zero = set) → RLE with maximal runs: no zero-length run behind the first."""
    p = np.asarray(plane)
    if p.ndim != 2:
        raise ValueError("rle_encode: a 2-D plane expected")
    h, w = p.shape
    flat = (p.T.reshape(-1) != 0).astype(np.int8)              # column-major
    edges = np.flatnonzero(np.diff(np.concatenate(([0], flat)))) if flat.size else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate(([0], edges, [h * w]))).astype(np.uint32)
    return {"size": [int(h), int(w)], "counts": counts}


def coco_results(image_ids: Sequence, det_src, rles, sizes, class_to_category: Optional[Dict[int, int]] = None,
                 score_threshold: float = 0.0, segmentation: str = "rle", min_area: int = 1, polygons=None,
                 tolerance: Optional[float] = None) -> List[Dict]:
    """The COCO results list (``segm`` results, which carry ``bbox`` too) of a batch: image_ids (B), det_src (B, rows, 6) — boxes
    normalized in each SOURCE image, as masks_rle_source returns them —, rles[b][i], sizes = [(h_b, w_b)].  One record per row with
    score > score_threshold: ``bbox`` is the detection's box in source pixels (Matterport's denorm_boxes of the row — the box the mask
    was pasted into — as x, y, width, height), ``category_id`` = class_to_category[class id] (the class id itself without a map),
    ``segmentation`` the RLE with its compressed string.  ``json.dumps`` takes the list as it is.

    segmentation="polygon" writes COCO's other form instead: a list of flat ``[x0, y0, x1, y1, ...]`` float lists, one per ring, in
    pixel-corner coordinates.  COCO polygons cannot carry holes, so this mode emits only the OUTLINES (the rings of positive area)
    of at least ``min_area`` pixels and DROPS the hole rings: a mask with a hole comes out filled, and a mask whose outlines are all
    smaller than min_area has an empty list.  ``polygons`` = what detection.rle_to_polygons or rle_to_polygons_host returned for
    ``rles`` (rings, areas); None traces them here with detection.rle_to_polygons, on the GPU.  ``tolerance`` (pixels) simplifies the
    rings (detection.simplify_polygons, on the GPU: while tracing here, or the ``polygons`` given; rings that are simplified already,
    such as rle_to_polygons_host(..., tolerance=) returns, are passed without it).  A ring is still chosen by its ORIGINAL area, the
    pixels it encloses; its simplified vertices are written, and a ring left with fewer than 3 vertices is dropped."""
    if segmentation not in ("rle", "polygon"):
        raise ValueError(f"coco_results: segmentation {segmentation!r} is neither 'rle' nor 'polygon'")
    if segmentation == "polygon" and polygons is None:
        from .detection import rle_to_polygons
        polygons = rle_to_polygons([[{"size": r["size"], "counts": _counts(r)} for r in row] for row in rles], sizes, tolerance=tolerance)
    elif segmentation == "polygon" and tolerance is not None:
        from .detection import simplify_polygons
        polygons = simplify_polygons(polygons, tolerance)
    det = np.asarray(det_src, dtype=np.float32)
    out = []
    for b, image_id in enumerate(image_ids):
        h, w = int(sizes[b][0]), int(sizes[b][1])
        for i in range(det.shape[1]):
            r = det[b, i]
            score = float(r[5])
            if not score > score_threshold:
                continue
            y1 = int(np.rint(float(r[0]) * (h - 1))); x1 = int(np.rint(float(r[1]) * (w - 1)))
            y2 = int(np.rint(float(r[2]) * (h - 1) + 1.0)); x2 = int(np.rint(float(r[3]) * (w - 1) + 1.0))
            cls = int(r[4])
            rle = rles[b][i]
            counts = rle["counts"]
            if segmentation == "polygon":
                seg = [[float(v) for v in ring.reshape(-1)] for ring, area in zip(polygons[0][b][i], polygons[1][b][i])
                       if area >= max(1, min_area) and len(ring) >= 3]
            else:
                seg = {"size": [int(rle["size"][0]), int(rle["size"][1])], "counts": counts if isinstance(counts, str) else rle_to_string(counts)}
            out.append({"image_id": image_id.item() if isinstance(image_id, np.generic) else image_id,
                        "category_id": int(class_to_category[cls]) if class_to_category is not None else cls,
                        "bbox": [float(x1), float(y1), float(x2 - x1), float(y2 - y1)],
                        "score": score,
                        "segmentation": seg})
    return out
