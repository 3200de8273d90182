"""Detections as a GeoJSON FeatureCollection (RFC 7946): the traced rings of every mask, nested into polygons of one exterior ring and
its holes by ``detection.nest_polygons``, with an affine geotransform.  Host-side and plain: the rings and their nesting come from the
library (``mrcnn_rle_to_polygons``, ``mrcnn_polygons_simplify``, ``mrcnn_polygons_nest``); this module only orders, orients and writes.

Simplification does not preserve topology: rings simplified with a tolerance may touch or cross themselves and one another, so a hole
may reach outside its shell.  The nesting written here is that of the TRACED rings, which simplification keeps one for one; trace
without a tolerance where a consumer validates geometry.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence

import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _ring(ring, transform, exterior: bool) -> List[List[float]]:
    """One ring of pixel corners -> closed GeoJSON positions: transformed in doubles, then oriented — an exterior to positive shoelace
    area, a hole to negative — keeping its first vertex, which is repeated at the end."""
    a, b, c, d, e, f = transform
    pts = [(a * float(x) + b * float(y) + c, d * float(x) + e * float(y) + f) for x, y in ring]
    twice = sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(pts, pts[1:] + pts[:1]))
    if (twice < 0) == exterior and twice != 0:
        pts = pts[:1] + pts[:0:-1]
    return [[x, y] for x, y in pts + pts[:1]]


def feature_collection(det_src, polygons, nest, sizes=None, class_names=None, transform=None, min_area: int = 1, image_ids=None,
                       props=None) -> Dict:
    """A FeatureCollection of a batch: det_src (B, slots, 6) source-frame rows, ``polygons`` = the nested (rings, areas) that
    detection.rle_to_polygons returned (simplified or not; the flat dictionaries are not taken), ``nest`` = what
    detection.nest_polygons returned for the nested form (None: the third entry of ``polygons``, as rle_to_polygons(..., nest=True)
    returns it).

    One Feature per row with score > 0 that has at least one shell left.  Its geometry is a ``Polygon`` for one shell — the exterior
    ring, then its holes — and a ``MultiPolygon`` for several; an island inside a hole is a polygon of its own.  Every ring is closed:
    its first position is repeated.  Properties: ``image`` (image_ids[b], or b), ``row``, ``category_id`` (the class id), ``category``
    (class_names[class id], when names are given), ``score``, ``bbox`` — x, y, width, height in source pixels: with ``sizes`` =
    [(h_b, w_b)] the detection's box as coco_results writes it, without sizes the bounding box of the written shells; ALWAYS in source
    pixels, never transformed, as ``area`` is the mask's pixels: the geometry alone goes through ``transform``.

    ``transform`` = (a, b, c, d, e, f) maps a pixel corner (x, y) to (a*x + b*y + c, d*x + e*y + f) in doubles, a GDAL-style
    geotransform; the default is the identity.  AFTER the transform, exteriors are oriented to positive shoelace area and holes to
    negative, reversing a ring where needed: RFC 7946's right-hand rule in the output frame.  A shell whose ORIGINAL pixel area is
    below ``min_area``, or that has fewer than 3 vertices left after simplification, is dropped with its holes; a hole with fewer
    than 3 vertices is dropped alone.

    ``props`` = the dictionary detection.rle_region_props (or predict_tiled(props=True)) returned for the same masks, entry b * slots +
    i for row i of image b: every Feature's properties then gain, after the keys above, ``centroid`` [x, y] and ``orientation``
    (radians, from +x towards +y) in source pixel corners like ``bbox``, ``perimeter`` (unit pixel edges), ``solidity`` and ``obb`` —
    the four corners of the minimum-area oriented box, which, being geometry, go through ``transform`` as the rings do.  Without
    props nothing changes.

    Simplification does not preserve topology: the nesting is the traced rings'; simplified rings may cross one another."""
    rings, areas = polygons[0], polygons[1]
    if nest is None:
        if len(polygons) < 3:
            raise ValueError("feature_collection: no nesting: pass nest_polygons' result, or rle_to_polygons(..., nest=True)")
        nest = polygons[2]
    groups = nest["nest"] if isinstance(nest, dict) else nest
    t = IDENTITY if transform is None else tuple(float(v) for v in transform)
    if len(t) != 6:
        raise ValueError("feature_collection: transform is (a, b, c, d, e, f)")
    det = np.asarray(det_src.cpu() if hasattr(det_src, "is_cuda") else det_src, dtype=np.float32)
    if det.ndim != 3 or det.shape[2] != 6 or det.shape[0] != len(rings) or any(len(row) != det.shape[1] for row in rings):
        raise ValueError(f"feature_collection: det_src {tuple(det.shape)} does not go with the rings")
    if props is not None and len(props["area"]) != det.shape[0] * det.shape[1]:
        raise ValueError(f"feature_collection: props of {len(props['area'])} masks do not go with det_src {tuple(det.shape)}")
    features = []
    for b in range(det.shape[0]):
        for i in range(det.shape[1]):
            row = det[b, i]
            if not float(row[5]) > 0.0:
                continue
            mine, mine_areas = rings[b][i], np.asarray(areas[b][i], dtype=np.int64)
            polys, corners = [], []
            for group in groups[b][i]:
                shell = int(group[0])
                if int(mine_areas[shell]) < max(1, int(min_area)) or len(mine[shell]) < 3:
                    continue
                corners.append(np.asarray(mine[shell]))
                polys.append([_ring(mine[shell], t, True)] + [_ring(mine[int(h)], t, False) for h in group[1:] if len(mine[int(h)]) >= 3])
            if not polys:
                continue
            if sizes is not None:
                h, w = int(sizes[b][0]), int(sizes[b][1])
                y1 = int(np.rint(float(row[0]) * (h - 1))); x1 = int(np.rint(float(row[1]) * (w - 1)))
                y2 = int(np.rint(float(row[2]) * (h - 1) + 1.0)); x2 = int(np.rint(float(row[3]) * (w - 1) + 1.0))
            else:
                every = np.concatenate(corners)
                x1, y1, x2, y2 = int(every[:, 0].min()), int(every[:, 1].min()), int(every[:, 0].max()), int(every[:, 1].max())
            cls = int(row[4])
            image = b if image_ids is None else image_ids[b]
            properties = {"image": image.item() if isinstance(image, np.generic) else image, "row": i, "category_id": cls}
            if class_names is not None:
                properties["category"] = str(class_names[cls])
            properties.update({"score": float(row[5]), "bbox": [float(x1), float(y1), float(x2 - x1), float(y2 - y1)], "area": int(mine_areas.sum())})
            if props is not None:
                k = b * det.shape[1] + i
                ta, tb, tc, td, te, tf = t
                properties.update({"centroid": [float(v) for v in props["centroid"][k]], "orientation": float(props["orientation"][k]),
                                   "perimeter": int(props["perimeter"][k]), "solidity": float(props["solidity"][k]),
                                   "obb": [[ta * float(x) + tb * float(y) + tc, td * float(x) + te * float(y) + tf] for x, y in props["obb_corners"][k]]})
            geometry = {"type": "Polygon", "coordinates": polys[0]} if len(polys) == 1 else {"type": "MultiPolygon", "coordinates": polys}
            features.append({"type": "Feature", "geometry": geometry, "properties": properties})
    return {"type": "FeatureCollection", "features": features}


def dumps(det_src, polygons, nest, **kwargs) -> bytes:
    """feature_collection(...) as deterministic bytes: the keys in the order they are written above, no spaces, the shortest decimal
    that gives each double back, UTF-8."""
    return json.dumps(feature_collection(det_src, polygons, nest, **kwargs), separators=(",", ":"), ensure_ascii=False, allow_nan=False).encode("utf-8")
