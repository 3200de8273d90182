"""Polygon ground truth encoded on the GPU (mrcnn_rle_from_polygons_batch) and kept there for scoring (COCOGroundTruth.to_device).
The expected value is always the unchanged host entry mrcnn_rle_from_polygons, called per annotation — never the code under test —
and every comparison is word for word."""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

from test_coco_eval_host import SMALL_SIZES, naive_score, synthetic_dataset

pytestmark = pytest.mark.gpu

SHAPE = 4
SENTINEL = 0x5A5A5A5A


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def host_set(anns, sizes):
    """The specification: mrcnn_rle_from_polygons per annotation -> (counts, run_offsets, areas, boxes of the decoded plane)."""
    CE = _mod("coco_eval")
    rles = [CE.rle_from_polygons(a, h, w) for a, (h, w) in zip(anns, sizes)]
    offs = np.zeros(len(rles) + 1, np.int64)
    offs[1:] = np.cumsum([r.size for r in rles])
    for r, (h, w) in zip(rles, sizes):
        assert int(r.astype(np.int64).sum()) == h * w                       # the host entry accepts every annotation
    counts = np.concatenate(rles).astype(np.uint32)
    areas = np.array([int(r[1::2].astype(np.int64).sum()) for r in rles], np.uint32)
    return counts, offs, areas, rles


def box_of_runs(r, h):
    """The tight box of the set pixels straight from the runs (column-major positions), 0,0,0,0 for none."""
    b = np.concatenate([[0], np.cumsum(r.astype(np.int64))])
    s, e = b[1:-1:2], b[2::2]
    keep = e > s
    s, e = s[keep], e[keep]
    if s.size == 0:
        return [0, 0, 0, 0]
    x0, x1 = s // h, (e - 1) // h
    multi = x1 > x0
    y0 = np.where(multi, 0, s % h); y1 = np.where(multi, h - 1, (e - 1) % h)
    return [int(x0.min()), int(y0.min()), int(x1.max() - x0.min() + 1), int(y1.max() - y0.min() + 1)]


def fixed_cases():
    """The cases of tests/test_coco_eval_host.py's polygon tests, as one batch."""
    rng = np.random.default_rng(0)
    anns, sizes = [], []

    def add(polys, h, w):
        anns.append([list(map(float, p)) for p in polys]); sizes.append((h, w))
    h, w = 37, 53
    for _ in range(60):                                                       # integer rectangles
        x0, x1 = sorted(rng.integers(0, w + 1, 2)); y0, y1 = sorted(rng.integers(0, h + 1, 2))
        add([[x0, y0, x1, y0, x1, y1, x0, y1]], h, w)
    add([[0, 0, w, 0, w, h, 0, h]], h, w)
    h, w = 30, 40
    add([[-10, -5, 12, -5, 12, 9, -10, 9]], h, w)                            # clipped
    add([[100, 100, 120, 100, 120, 130, 100, 130]], h, w)                    # wholly outside
    add([[-50, -50, -20, -50, -20, -10]], h, w)
    a = [3.2, 4.1, 25.7, 6.3, 20.2, 22.8, 6.6, 18.4]
    b = [15.5, 10.5, 38.2, 12.1, 30.9, 28.3]
    add([a], h, w); add([b], h, w); add([a, b], h, w); add([b, a], h, w)       # union in both orders
    pts = np.array(a).reshape(-1, 2)
    for k in range(4):                                                        # rotated and reversed vertex order
        rot = np.roll(pts, k, axis=0)
        add([rot.reshape(-1).tolist()], h, w); add([rot[::-1].reshape(-1).tolist()], h, w)
    for poly in ([], [5, 5], [5, 5, 20, 9], [5, 5, 5, 5, 5, 5], [2, 3, 12, 3, 22, 3]):    # the five degenerate polygons
        add([poly], h, w)
    add([], h, w)                                                             # an annotation with no polygon
    return anns, sizes


def random_cases(n=2200, seed=17):
    """Seeded: sizes from 1x1 over odd mixed sizes to a side of 32767; 1-6 polygons; 3-400 vertices; fractional coordinates, some
    within 1e-9 of a rounding tie of the x5 grid; vertices outside the plane; self-intersecting outlines (random vertex order);
    near-vertical and near-horizontal edges; and annotations whose toggles exceed the LDS path's limit."""
    rng = np.random.default_rng(seed)
    anns, sizes = [], []
    for it in range(n):
        mode = it % 11
        if it < 4:
            h, w = [(1, 1), (1, 7), (5, 1), (2, 2)][it]
        elif it % 211 == 7:
            h, w = 32767, int(rng.integers(1, 12))
        elif it % 211 == 9:
            h, w = int(rng.integers(1, 12)), 32767
        elif mode == 0:
            h, w = int(rng.integers(200, 700)) | 1, int(rng.integers(200, 900)) | 1
        else:
            h, w = int(rng.integers(1, 140)), int(rng.integers(1, 180))
        polys = []
        for _ in range(int(rng.integers(1, 7))):
            k = int(rng.integers(3, 401)) if mode == 1 else int(rng.integers(3, 25))
            style = int(rng.integers(0, 6))
            cx, cy, r = rng.uniform(-0.2, 1.2) * w, rng.uniform(-0.2, 1.2) * h, rng.uniform(0.5, 0.7) * max(h, w)
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            if style == 0:                                                    # any order: self-intersecting, partly outside
                x, y = rng.uniform(-0.4, 1.4, k) * w, rng.uniform(-0.4, 1.4, k) * h
            elif style == 1:                                                  # a simple outline around a centre
                rr = r * rng.uniform(0.3, 1.0, k)
                x, y = cx + rr * np.cos(ang), cy + rr * np.sin(ang)
            elif style == 2:                                                  # integer corners
                x, y = np.floor(rng.uniform(-2, w + 3, k)), np.floor(rng.uniform(-2, h + 3, k))
            elif style == 3:                                                  # scaled values within 1e-9 of a rounding tie
                x = (np.floor(rng.uniform(-10, 5 * w + 10, k)) + .5) / 5.0 + rng.integers(-1, 2, k) * rng.uniform(0, 1.9e-10, k)
                y = (np.floor(rng.uniform(-10, 5 * h + 10, k)) + .5) / 5.0 + rng.integers(-1, 2, k) * rng.uniform(0, 1.9e-10, k)
            elif style == 4:                                                  # near-vertical edges
                x = np.repeat(rng.uniform(0, w, (k + 1) // 2), 2)[:k] + rng.uniform(-1e-3, 1e-3, k)
                y = rng.uniform(-0.2, 1.2, k) * h
            else:                                                             # near-horizontal edges
                y = np.repeat(rng.uniform(0, h, (k + 1) // 2), 2)[:k] + rng.uniform(-1e-3, 1e-3, k)
                x = rng.uniform(-0.2, 1.2, k) * w
            polys.append(np.stack([x, y], 1).reshape(-1).tolist())
        anns.append(polys); sizes.append((h, w))
    # past the LDS limit: a zigzag of 60 vertices across a wide plane, and one across a side of 32767
    for h, w, k in ((64, 2001, 60), (9, 32767, 14)):
        x = np.where(np.arange(k) % 2 == 0, 0.3, w - 0.7) + np.arange(k) * 0.01
        y = np.linspace(0.2, h - 0.4, k)
        anns.append([np.stack([x, y], 1).reshape(-1).tolist(), [1.5, 1.5, w / 2, h - 1.2, w - 2.5, 2.25]]); sizes.append((h, w))
    return anns, sizes


def _assert_same_set(got, want, sizes):
    counts, offs, areas, boxes = got
    w_counts, w_offs, w_areas, w_rles = want
    np.testing.assert_array_equal(np.asarray(offs), w_offs)
    np.testing.assert_array_equal(np.asarray(counts).view(np.uint32), w_counts)
    np.testing.assert_array_equal(np.asarray(areas).view(np.uint32), w_areas)
    np.testing.assert_array_equal(np.asarray(boxes), np.array([box_of_runs(r, h) for r, (h, w) in zip(w_rles, sizes)], np.int32).reshape(-1, 4))


def test_the_host_cases_as_one_batch():
    CE, CR = _mod("coco_eval"), _mod("coco_results")
    anns, sizes = fixed_cases()
    want = host_set(anns, sizes)
    got = CE.rle_from_polygons_batch(anns, sizes)
    _assert_same_set(got, want, sizes)
    counts, offs, areas, boxes = got
    for k, (h, w) in enumerate(sizes):
        r = counts[offs[k]:offs[k + 1]]
        assert int(areas[k]) == int(r[1::2].astype(np.int64).sum())          # the sum of the odd runs
        plane = CR.rle_decode({"size": [h, w], "counts": r})
        ys, xs = np.nonzero(plane)
        tight = [0, 0, 0, 0] if ys.size == 0 else [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert list(boxes[k]) == [int(v) for v in tight], k                   # the tight box of the decoded plane
    assert list(counts[offs[-2]:offs[-1]]) == [30 * 40]                       # no polygon: the single run [h*w]
    assert (areas[:60] > 0).any() and int(areas[62]) == 0


def test_random_set_word_for_word_on_both_sort_paths():
    CE = _mod("coco_eval")
    anns, sizes = random_cases()
    assert len(anns) >= 2000
    want = host_set(anns, sizes)
    got = CE.rle_from_polygons_batch(anns, sizes)
    _assert_same_set(got, want, sizes)
    # both sort paths ran: an RLE of r runs has at least r - 1 toggles, so more runs than the limit + 1 went the global way; an
    # annotation whose edges cannot cross LDS_TOGGLES column centres (edges x width) went through LDS
    runs = np.diff(want[1])
    edges = np.array([sum(len(p) // 2 for p in a) for a in anns])
    widths = np.array([w for _, w in sizes])
    n_global, n_lds = int((runs > CE.LDS_TOGGLES + 1).sum()), int((edges * widths <= CE.LDS_TOGGLES).sum())
    print("annotations", len(anns), "runs", int(runs.sum()), "surely global", n_global, "surely LDS", n_lds, "largest RLE", int(runs.max()))
    assert n_global >= 2 and n_lds >= 200
    assert max(max(s) for s in sizes) == 32767 and min(min(s) for s in sizes) == 1
    assert max(len(p) // 2 for a in anns for p in a) > 300 and max(len(a) for a in anns) == 6


def test_memspaces_agree_and_the_capacity_protocol():
    import torch
    CE, lib = _mod("coco_eval"), _mod("_lib")
    L = lib.lib()
    anns, sizes = random_cases(n=300, seed=5)
    host = CE.rle_from_polygons_batch(anns, sizes)
    dev = CE.rle_from_polygons_batch(anns, sizes, device="cuda")
    assert all(t.is_cuda for t in dev)
    for a, b in zip(host, dev):
        np.testing.assert_array_equal(np.asarray(a).view(np.int32) if a.dtype == np.uint32 else np.asarray(a), b.cpu().numpy())
    need = int(host[1][-1])
    # the raw protocol, host and device
    polys = [np.asarray(p, np.float64) for a in anns for p in a]
    xy = np.ascontiguousarray(np.concatenate(polys))
    po = np.zeros(len(polys) + 1, np.int64); po[1:] = np.cumsum([p.size // 2 for p in polys])
    ao = np.zeros(len(anns) + 1, np.int64); ao[1:] = np.cumsum([len(a) for a in anns])
    hs = np.array([s[0] for s in sizes], np.int32); ws = np.array([s[1] for s in sizes], np.int32)
    n = len(anns)
    for space in ("host", "device"):
        if space == "host":
            counts = np.full(need, SENTINEL, np.uint32); ro = np.zeros(n + 1, np.int64); ar = np.zeros(n, np.uint32)
            ptr = lambda a: a.ctypes.data
            back = lambda a: a
        else:
            counts = torch.full((need,), SENTINEL, dtype=torch.int32, device="cuda"); ro = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            ar = torch.zeros(n, dtype=torch.int32, device="cuda")
            ptr = lambda a: a.data_ptr()
            back = lambda a: a.cpu().numpy()
        sp = lib.HOST if space == "host" else lib.DEVICE
        call = lambda c, cap: L.mrcnn_rle_from_polygons_batch(xy.ctypes.data, po.ctypes.data, ao.ctypes.data, n, hs.ctypes.data, ws.ctypes.data, sp,
                                                              c, cap, ptr(ro), ptr(ar), None)
        assert call(None, 0) == SHAPE                                            # the size query
        msg = L.mrcnn_last_error().decode()
        assert f"capacity >= {need}" in msg, msg
        np.testing.assert_array_equal(back(ro), host[1])                          # offsets and areas are written all the same
        np.testing.assert_array_equal(back(ar).view(np.uint32), host[2])
        assert call(ptr(counts), need - 1) == SHAPE and f"capacity >= {need}" in L.mrcnn_last_error().decode()
        assert (back(counts).view(np.uint32) == SENTINEL).all()                   # counts untouched
        assert call(ptr(counts), need) == 0
        np.testing.assert_array_equal(back(counts).view(np.uint32), host[0])
    # no annotation at all
    ro = np.full(1, 7, np.int64)
    assert L.mrcnn_rle_from_polygons_batch(None, None, ao.ctypes.data, 0, None, None, lib.HOST, None, 0, ro.ctypes.data, None, None) == 0 and ro[0] == 0


def _polygon_dataset(compressed, seed):
    """synthetic_dataset with polygon annotations added (some without `area`), its crowds in one of the two RLE forms."""
    ds, res = synthetic_dataset(SMALL_SIZES, seed=seed, compressed=compressed)
    rng = np.random.default_rng(seed)
    aid = 10000
    for im in ds["images"][:-2]:
        h, w = im["height"], im["width"]
        for j in range(3):
            k = int(rng.integers(5, 40))
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rr = rng.uniform(0.4, 1.0, k)
            cx, cy = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h
            p = np.stack([cx + 0.4 * w * rr * np.cos(ang), cy + 0.4 * h * rr * np.sin(ang)], 1).reshape(-1).tolist()
            polys = [p] if j else [p, [1.0, 1.0, w / 3, 2.0, w / 4, h / 2]]
            ds["annotations"].append({"id": aid, "image_id": im["id"], "category_id": 1 + j, "iscrowd": 0, "area": None if j == 1 else 0.3 * h * w,
                                      "bbox": [1.0, 1.0, w / 2, h / 2], "segmentation": polys})
            aid += 1
    order = np.random.default_rng(seed + 1).permutation(len(ds["annotations"]))        # polygons and RLE forms interleaved
    ds["annotations"] = [ds["annotations"][i] for i in order]
    return ds, res


def _same_scores(a, b):
    for k in ("precision", "recall", "stats"):
        assert np.array_equal(a[k], b[k]), k
    assert len(a["stats"]) == 12


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_scoring_with_resident_ground_truth(iou_type):
    CE = _mod("coco_eval")
    crowds = 0
    for compressed in (False, True):
        ds, res = _polygon_dataset(compressed, seed=5 + int(compressed))
        crowds += sum(a["iscrowd"] for a in ds["annotations"])
        plain = CE.score(CE.COCOGroundTruth(ds), res, iou_type)
        gt = CE.COCOGroundTruth(ds)
        resident = gt.to_device()
        assert resident.counts.is_cuda and resident.run_offsets.is_cuda and resident.areas.is_cuda and resident.n == len(ds["annotations"])
        # the resident set is the host encoding of every annotation, in by_image order
        order = [a for anns in gt.by_image.values() for a in anns]
        ref = CE.COCOGroundTruth(ds)
        offs = resident.run_offsets.cpu().numpy(); counts = resident.counts.cpu().numpy().view(np.uint32)
        for k, a in enumerate(order):
            twin = next(b for b in ref.annotations if b["id"] == a["id"])
            np.testing.assert_array_equal(counts[offs[k]:offs[k + 1]], ref.counts(twin))
        _same_scores(plain, CE.score(gt, res, iou_type, device_gt=resident))
        sub = [im["id"] for im in ds["images"]][1:4]
        _same_scores(CE.score(CE.COCOGroundTruth(ds), res, iou_type, img_ids=sub), CE.score(gt, res, iou_type, img_ids=sub, device_gt=resident))
        assert 0.0 < plain["stats"][0] < 1.0
    assert crowds > 0


def _device_batches(seed=31):
    """Two device batches of two images (mrcnn_masks_rle_source's buffers) and a ground truth of polygons and crowds in both RLE forms."""
    import torch
    CE, CR, D, E = _mod("coco_eval"), _mod("coco_results"), _mod("detection"), _mod("evaluate")
    rng = np.random.default_rng(seed)
    sizes = [(480, 640), (427, 640), (640, 480), (375, 500)]
    H, W, rows = 256, 320, 20
    B = len(sizes)
    det = np.zeros((B, rows, 6), np.float32)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    masks = np.zeros((B, rows, 28, 28), np.float32)
    for b, (h, w) in enumerate(sizes):
        nh, nw, py, px = E.letterbox_geometry(h, w, H, W)
        for i in range(rows - 3):
            y1 = (py + rng.uniform(0, 0.6) * nh) / (H - 1); x1 = (px + rng.uniform(0, 0.6) * nw) / (W - 1)
            det[b, i] = [y1, x1, min(1.0, y1 + rng.uniform(0.05, 0.4) * nh / H), min(1.0, x1 + rng.uniform(0.05, 0.4) * nw / W), rng.integers(1, 4),
                         0.3 + 0.6 * rng.random()]
            cy, cx, sy, sx = rng.uniform(8, 20), rng.uniform(8, 20), rng.uniform(4, 12), rng.uniform(4, 12)
            masks[b, i] = np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
    image_ids = [40, 30, 20, 10]
    det_src, rles, areas, _ = D.masks_rle_source(det, masks, sizes, H, W, 0.5)
    results = CR.coco_results(image_ids, det_src, rles, sizes)
    anns = []
    for k, r in enumerate(results[::2]):
        x, y, bw, bh = r["bbox"]
        ann = {"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "area": None if k % 4 == 0 else float(bw * bh),
               "bbox": list(r["bbox"])}
        if k % 5 == 3:                                                              # a crowd, in one of the two RLE forms
            plane = CR.rle_decode(r["segmentation"])
            c = CR.rle_encode(plane)["counts"]
            ann.update(iscrowd=1, area=float(plane.sum()),
                       segmentation={"size": list(plane.shape), "counts": CR.rle_to_string(c) if k % 10 == 3 else [int(v) for v in c]})
        else:                                                                       # an octagon inside the detection's box
            t = np.linspace(0, 2 * np.pi, 8, endpoint=False) + 0.1 * k
            ann["segmentation"] = [np.stack([x + bw / 2 + 0.45 * bw * np.cos(t), y + bh / 2 + 0.45 * bh * np.sin(t)], 1).reshape(-1).tolist()]
        anns.append(ann)
    ds = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(image_ids, sizes)], "categories": [{"id": c} for c in (1, 2, 3)], "annotations": anns}
    batches = [CE.device_detections(image_ids[s:s + 2], torch.from_numpy(det[s:s + 2]).cuda(), torch.from_numpy(masks[s:s + 2]).cuda(), sizes[s:s + 2], H, W, 0.5)
               for s in (0, 2)]
    return ds, results, batches


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_score_batch_reads_the_resident_buffers(iou_type, monkeypatch):
    CE, lib = _mod("coco_eval"), _mod("_lib")
    ds, results, batches = _device_batches()
    forms = [type(a["segmentation"]["counts"]) for a in ds["annotations"] if a["iscrowd"]]
    assert str in forms and list in forms and any(not a["iscrowd"] for a in ds["annotations"])
    plain = CE.score_batch(CE.COCOGroundTruth(ds), batches, iou_type)
    _same_scores(plain, CE.score(CE.COCOGroundTruth(ds), results, iou_type))
    assert 0.0 < plain["stats"][0] <= 1.0
    gt = CE.COCOGroundTruth(ds)
    resident = gt.to_device()
    L = lib.lib()
    real, seen = L.mrcnn_rle_iou, []

    def spy(*args):
        seen.append((int(args[3] or 0), int(args[4] or 0), int(args[5])))
        return real(*args)
    monkeypatch.setattr(L, "mrcnn_rle_iou", spy)
    with_resident = CE.score_batch(gt, batches, iou_type, device_gt=resident)
    _same_scores(plain, with_resident)
    if iou_type == "segm":
        lo = resident.counts.data_ptr()
        hi = lo + 4 * int(resident.counts.numel())
        assert len(seen) == len(batches)
        olo = resident.run_offsets.data_ptr()
        for g_counts, g_offsets, n_g in seen:                                     # no upload per batch: the resident buffers themselves
            assert lo <= g_counts < hi and olo <= g_offsets and g_offsets + 8 * (n_g + 1) <= olo + 8 * (resident.n + 1) and 0 < n_g <= resident.n
        # a category filter that breaks an image's range: the gather fallback, still without the host, and the same numbers
        seen.clear()
        ds2 = dict(ds, categories=[{"id": c} for c in (1, 3)])
        gt2 = CE.COCOGroundTruth(ds2)
        r2 = gt2.to_device()
        _same_scores(CE.score_batch(CE.COCOGroundTruth(ds2), batches, iou_type), CE.score_batch(gt2, batches, iou_type, device_gt=r2))
        assert seen and all(n_g < r2.n for _, _, n_g in seen[-len(batches):])
    else:
        assert not seen


def test_evaluate_coco_scored_with_resident_ground_truth(pkg, small_model, tmp_path):
    CE, CR, E = _mod("coco_eval"), _mod("coco_results"), _mod("evaluate")
    d, cfg = small_model
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    sizes = [(96, 160), (300, 200), (128, 128), (37, 53), (64, 427), (333, 100), (200, 201)]
    rng = np.random.default_rng(11)
    pixels = {50 - i: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)}
    items = [(i, p) for i, p in pixels.items()]
    _, _, _, first = E.evaluate_segm(m, items, limit=None, verbose=False, batch=4)
    anns = []
    for k, r in enumerate(first):
        plane = CR.rle_decode(r["segmentation"])
        if plane.sum() == 0:
            continue
        x, y, bw, bh = r["bbox"]
        if k % 2:                                                                  # the detection's own mask, as RLE
            seg, area = {"size": r["segmentation"]["size"], "counts": r["segmentation"]["counts"]}, float(plane.sum())
        else:                                                                      # its box, as a polygon
            seg, area = [[x, y, x + bw, y, x + bw, y + bh, x, y + bh]], None
        anns.append({"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "area": area, "bbox": r["bbox"],
                     "segmentation": seg})
    assert any(isinstance(a["segmentation"], list) for a in anns) and any(isinstance(a["segmentation"], dict) for a in anns)
    cats = sorted(set(a["category_id"] for a in anns))
    ds = {"images": [{"id": i, "height": p.shape[0], "width": p.shape[1], "file_name": f"{i}.png", "coco_url": "", "flickr_url": "",
                      "date_captured": "", "license": 0} for i, p in pixels.items()],
          "categories": [{"id": c, "name": str(c), "supercategory": ""} for c in cats], "annotations": anns, "info": {}, "licenses": []}
    path = str(tmp_path / "gt.json")
    with open(path, "w") as f:
        json.dump(ds, f)
    plain = E.evaluate_coco_scored(m, path, lambda im: pixels[im.id], limit=7, verbose=False, batch=4)
    resident = E.evaluate_coco_scored(m, path, lambda im: pixels[im.id], limit=7, verbose=False, batch=4, device_gt=True)
    for iou_type in ("segm", "bbox"):
        _same_scores(plain[4][iou_type], resident[4][iou_type])
        assert plain[4][iou_type]["stats"][0] > 0.0
        print(iou_type, "AP", plain[4][iou_type]["stats"][0], "annotations", len(anns))
