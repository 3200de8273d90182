"""COCO scoring, the half that needs no GPU: mrcnn_rle_from_polygons, COCOGroundTruth, accumulate / summarize — and the YARDSTICK
of tests/test_gpu_coco_eval.py: COCO's published evaluation procedure (COCOeval: computeIoU, evaluateImg, accumulate, summarize)
restated as naively as possible — dense uint8 planes, Python loops, ``(a & b).sum()``, one function per step.  It shares no code
with coco_eval.py or the library (coco_results.rle_decode only turns an RLE into its plane).  pycocotools itself is not available
where this suite runs, so nobody has compared either leg with it yet; the one deliberate difference of both legs: "matched" is
tested as matched, not as "ground-truth id > 0"."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


# ==================================================================================================================================
# the naive leg
# ==================================================================================================================================
N_IOU_THRS = [0.5 + 0.05 * i for i in range(10)]          # only used to build COCO's own linspace below
N_AREA = [[0.0, 1e10], [0.0, 1024.0], [1024.0, 9216.0], [9216.0, 1e10]]
N_MAXDETS = [1, 10, 100]


def naive_thresholds():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True), np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def naive_mask_iou(d_planes, g_planes, crowd):
    """(nd, ng) inter (python ints) and iou (float64): (a & b).sum(), crowd rule inter / area_d, 0 / 0 = 0."""
    inter = [[0] * len(g_planes) for _ in d_planes]
    iou = np.zeros((len(d_planes), len(g_planes)), np.float64)
    for i, d in enumerate(d_planes):
        for j, g in enumerate(g_planes):
            it = int((d.astype(bool) & g.astype(bool)).sum())
            ad, ag = int(d.astype(bool).sum()), int(g.astype(bool).sum())
            den = ad if crowd[j] else ad + ag - it
            inter[i][j] = it
            iou[i, j] = np.float64(it) / np.float64(den) if den else 0.0
    return inter, iou


def naive_box_iou(d_boxes, g_boxes, crowd):
    iou = np.zeros((len(d_boxes), len(g_boxes)), np.float64)
    for i, d in enumerate(d_boxes):
        for j, g in enumerate(g_boxes):
            d = [np.float64(v) for v in d]; g = [np.float64(v) for v in g]
            w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
            h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
            if w <= 0 or h <= 0:
                continue
            it = w * h
            u = d[2] * d[3] if crowd[j] else d[2] * d[3] + g[2] * g[3] - it
            iou[i, j] = it / u if u != 0 else 0.0
    return iou


def naive_evaluate_img(ious, dt_areas, gt_areas, gt_crowd, area_rng, thrs):
    """COCOeval.evaluateImg for one (image, category) and one area range.  ious (nd, ng): detections in score order (already cut to
    maxDet), ground truths in annotation order.  Returns dtm (T, nd) — the position in the annotation-order list of the ground truth
    taken, or -1 —, dt_ig (T, nd), gtm (T, ng) — position of the detection, or -1 —, gt_ig (ng) in annotation order."""
    nd, ng = len(dt_areas), len(gt_areas)
    ig = [1 if (gt_crowd[j] or gt_areas[j] < area_rng[0] or gt_areas[j] > area_rng[1]) else 0 for j in range(ng)]
    order = sorted(range(ng), key=lambda j: ig[j])                   # python's sort is stable: non-ignored first
    T = len(thrs)
    dtm = [[-1] * nd for _ in range(T)]
    dt_ig = [[0] * nd for _ in range(T)]
    gtm = [[-1] * ng for _ in range(T)]
    for t, thr in enumerate(thrs):
        for d in range(nd):
            bar = min(thr, 1 - 1e-10)
            m = -1
            for pos, j in enumerate(order):
                if gtm[t][j] >= 0 and not gt_crowd[j]:
                    continue
                if m > -1 and ig[order[m]] == 0 and ig[j] == 1:
                    break
                if ious[d][j] < bar:
                    continue
                bar = ious[d][j]
                m = pos
            if m == -1:
                continue
            j = order[m]
            dt_ig[t][d] = ig[j]
            dtm[t][d] = j
            gtm[t][j] = d
        for d in range(nd):
            if dtm[t][d] == -1 and (dt_areas[d] < area_rng[0] or dt_areas[d] > area_rng[1]):
                dt_ig[t][d] = 1
    return dtm, dt_ig, gtm, ig


def naive_accumulate(E_by_cat, n_thrs, rec_thrs, max_dets=N_MAXDETS, n_areas=4):
    """COCOeval.accumulate.  E_by_cat[k] = per image (in image order) a dict: scores [nd], and per area range a: dtm[a][t][d] (>= 0 =
    matched), dt_ig[a][t][d], gt_ig[a][j]."""
    T, R, K, A, M = n_thrs, len(rec_thrs), len(E_by_cat), n_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        E = E_by_cat[k]
        if len(E) == 0:
            continue
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                entries = []                                  # (score, image position, detection position) — one per kept detection
                for ei, e in enumerate(E):
                    for d in range(min(max_det, len(e["scores"]))):
                        entries.append((e["scores"][d], ei, d))
                order = sorted(range(len(entries)), key=lambda i: -entries[i][0])          # stable
                npig = sum(1 for e in E for v in e["gt_ig"][a] if v == 0)
                if npig == 0:
                    continue
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for i in order:
                        _, ei, d = entries[i]
                        matched = E[ei]["dtm"][a][t][d] >= 0
                        ignored = E[ei]["dt_ig"][a][t][d] != 0
                        if matched and not ignored:
                            tp += 1
                        if (not matched) and not ignored:
                            fp += 1
                        rc.append(np.float64(tp) / npig)
                        pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.spacing(1)))
                    nd = len(order)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, r in enumerate(rec_thrs):
                        pi = 0
                        while pi < nd and rc[pi] < r:         # searchsorted(..., side="left"): the first recall >= r
                            pi += 1
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def naive_summarize(precision, recall, thrs, max_dets=N_MAXDETS):
    def one(ap, iou_thr=None, a=0, m=2):
        s = precision if ap else recall
        ts = range(len(thrs)) if iou_thr is None else [i for i, v in enumerate(thrs) if v == iou_thr]
        vals = []
        for t in ts:
            block = s[t, :, :, a, m] if ap else s[t, :, a, m]
            vals += [v for v in np.asarray(block).reshape(-1) if v > -1]
        return -1.0 if not vals else float(np.mean(np.array(vals)))
    return np.array([one(1), one(1, .5), one(1, .75), one(1, a=1), one(1, a=2), one(1, a=3), one(0, m=0), one(0, m=1), one(0, m=2),
                     one(0, a=1), one(0, a=2), one(0, a=3)])


def naive_score(dataset: dict, results: list, iou_type: str, img_ids=None):
    """The whole procedure on a COCO dataset dict whose segmentations are RLE dicts, and COCO result records.  Returns precision,
    recall, stats and `per` = {(image, category): the evaluateImg tables} for the matching comparison."""
    CR = _mod("coco_results")
    thrs, rec_thrs = naive_thresholds()
    imgs = sorted(im["id"] for im in dataset["images"]) if img_ids is None else sorted(set(img_ids))
    cats = sorted(c["id"] for c in dataset["categories"])
    per = {}
    E_by_cat = []
    for cat in cats:
        E = []
        for img in imgs:
            gts = [a for a in dataset["annotations"] if a["image_id"] == img and a["category_id"] == cat]
            dts = [r for r in results if r["image_id"] == img and r["category_id"] == cat]
            if not gts and not dts:
                continue
            dts = [dts[i] for i in sorted(range(len(dts)), key=lambda i: -dts[i]["score"])][:N_MAXDETS[-1]]
            crowd = [int(a.get("iscrowd", 0)) for a in gts]
            if iou_type == "segm":
                dp = [CR.rle_decode(r["segmentation"]) for r in dts]
                gp = [CR.rle_decode(a["segmentation"]) for a in gts]
                _, ious = naive_mask_iou(dp, gp, crowd)
                dt_areas = [float(p.sum()) for p in dp]
            else:
                ious = naive_box_iou([r["bbox"] for r in dts], [a["bbox"] for a in gts], crowd)
                dt_areas = [float(r["bbox"][2]) * float(r["bbox"][3]) for r in dts]
            gt_areas = [float(a["area"]) for a in gts]
            e = {"scores": [r["score"] for r in dts], "dtm": [], "dt_ig": [], "gtm": [], "gt_ig": []}
            for rng in N_AREA:
                dtm, dt_ig, gtm, ig = naive_evaluate_img(ious, dt_areas, gt_areas, crowd, rng, thrs)
                e["dtm"].append(dtm); e["dt_ig"].append(dt_ig); e["gtm"].append(gtm); e["gt_ig"].append(ig)
            per[(img, cat)] = e
            E.append(e)
        E_by_cat.append(E)
    precision, recall = naive_accumulate(E_by_cat, len(thrs), rec_thrs)
    return {"precision": precision, "recall": recall, "stats": naive_summarize(precision, recall, thrs), "per": per}


# ==================================================================================================================================
# synthetic data shared with the GPU tests
# ==================================================================================================================================
def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - cy) / max(ry, 1e-9)) ** 2 + ((xx - cx) / max(rx, 1e-9)) ** 2) <= 1.0).astype(np.uint8)


def tight_box(plane):
    ys, xs = np.nonzero(plane)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def synthetic_dataset(sizes, seed=5, compressed=False):
    """Ground truth + detections on small planes.  Categories 1, 2, 3 carry objects, 4 none at all (only detections), 5 only ground
    truth.  Per image: ellipses of areas on both sides of 32^2 and 96^2 where the plane allows, a noisy one, an empty one, a crowd;
    detections = shifted / eroded copies, exact copies (IoU 1), halves (IoU exactly 0.5), three quarters (0.75), duplicates,
    wrong-category copies, pure false positives, equal scores.  Image ids descend; the last two images: detections without ground
    truth, ground truth without detections; image 0 gets > 100 detections of category 1."""
    CR = _mod("coco_results")
    rng = np.random.default_rng(seed)
    images, anns, results = [], [], []
    aid = 1

    def seg(plane):
        r = CR.rle_encode(plane)
        return {"size": r["size"], "counts": CR.rle_to_string(r["counts"]) if compressed else [int(v) for v in r["counts"]]}

    def add_gt(img, cat, plane, crowd=0):
        nonlocal aid
        anns.append({"id": aid, "image_id": img, "category_id": cat, "iscrowd": crowd, "area": float(plane.sum()), "bbox": tight_box(plane),
                     "segmentation": seg(plane)})
        aid += 1

    def add_dt(img, cat, plane, score):
        r = CR.rle_encode(plane)
        results.append({"image_id": img, "category_id": cat, "score": float(score), "bbox": tight_box(plane),
                        "segmentation": {"size": r["size"], "counts": CR.rle_to_string(r["counts"])}})

    n = len(sizes)
    for k, (h, w) in enumerate(sizes):
        img = 1000 - 7 * k
        images.append({"id": img, "height": h, "width": w, "file_name": f"{img}.png"})
        if k == n - 2:                                           # detections, no ground truth
            add_dt(img, 1, ellipse(h, w, h / 2, w / 2, h / 4, w / 4), 0.6)
            add_dt(img, 2, ellipse(h, w, h / 3, w / 3, h / 5, w / 5), 0.55)
            continue
        planes = []
        for j in range(6):
            cat = 1 + j % 3
            ry, rx = rng.uniform(0.05, 0.45) * h, rng.uniform(0.05, 0.45) * w
            p = ellipse(h, w, rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w, ry, rx)
            if j == 3:
                p = (p & (rng.random((h, w)) < 0.7)).astype(np.uint8)            # noisy
            if j == 4:
                p = np.zeros((h, w), np.uint8)                                    # empty
            add_gt(img, cat, p, crowd=1 if j == 5 else 0)
            planes.append((cat, p))
        add_gt(img, 5, ellipse(h, w, h / 2, w / 2, 3, 3))
        # rectangles whose halves / three quarters give IoU exactly 0.5 / 0.75
        rect = np.zeros((h, w), np.uint8); rect[2:2 + 8, 1:1 + 8] = 1
        add_gt(img, 2, rect)
        planes.append((2, rect))
        if k == n - 1:                                           # ground truth, no detections
            continue
        half = rect.copy(); half[2:10, 5:9] = 0
        tq = rect.copy(); tq[2:10, 7:9] = 0
        add_dt(img, 2, half, 0.81); add_dt(img, 2, tq, 0.80); add_dt(img, 2, rect, 0.79)
        for cat, p in planes[:6]:
            sh = np.roll(np.roll(p, int(rng.integers(-3, 4)), 0), int(rng.integers(-3, 4)), 1)
            er = p.copy(); er[::3] = 0
            add_dt(img, cat, sh, rng.uniform(0.3, 0.99))
            add_dt(img, cat, er, 0.5)                              # equal scores
            add_dt(img, cat, p, 0.5)                               # exact copy, a duplicate of the object
            add_dt(img, 1 + cat % 3, p, rng.uniform(0.3, 0.9))     # wrong category
            add_dt(img, 4, p, rng.uniform(0.3, 0.9))               # a category without any ground truth
        add_dt(img, 1, ellipse(h, w, 2, 2, 2, 2), 0.95)            # pure false positives
        add_dt(img, 3, (rng.random((h, w)) < 0.02).astype(np.uint8), 0.2)
        if k == 0:
            base = planes[0][1]
            for i in range(110):
                add_dt(img, 1, np.roll(base, i % 5 - 2, 1), 0.9 - 0.005 * i)
    dataset = {"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in (1, 2, 3, 4, 5)]}
    return dataset, results


SMALL_SIZES = [(40, 56), (130, 120), (64, 33), (25, 90), (48, 48), (30, 30)]


# ==================================================================================================================================
# mrcnn_rle_from_polygons
# ==================================================================================================================================
def _poly_plane(polys, h, w):
    CE, CR = _mod("coco_eval"), _mod("coco_results")
    c = CE.rle_from_polygons(polys, h, w)
    assert int(c.astype(np.int64).sum()) == h * w
    assert np.all(c[1:] > 0), "a zero-length run behind the first"
    return CR.rle_decode({"size": [h, w], "counts": c})


def test_rectangles_are_exact():
    """[x0,y0, x1,y0, x1,y1, x0,y1] with integer corners sets exactly x0 <= x < x1, y0 <= y < y1 — what rleFrBbox relies on."""
    rng = np.random.default_rng(0)
    h, w = 37, 53
    for _ in range(60):
        x0, x1 = sorted(rng.integers(0, w + 1, 2)); y0, y1 = sorted(rng.integers(0, h + 1, 2))
        want = np.zeros((h, w), np.uint8); want[y0:y1, x0:x1] = 1
        got = _poly_plane([[x0, y0, x1, y0, x1, y1, x0, y1]], h, w)
        np.testing.assert_array_equal(got, want, err_msg=f"{x0},{y0},{x1},{y1}")
        assert int(got.sum()) == (x1 - x0) * (y1 - y0)
    np.testing.assert_array_equal(_poly_plane([[0, 0, w, 0, w, h, 0, h]], h, w), np.ones((h, w), np.uint8))


def test_polygons_clip_union_order_degenerate():
    h, w = 30, 40
    # clipped, not an error
    part = _poly_plane([[-10, -5, 12, -5, 12, 9, -10, 9]], h, w)
    want = np.zeros((h, w), np.uint8); want[0:9, 0:12] = 1
    np.testing.assert_array_equal(part, want)
    assert _poly_plane([[100, 100, 120, 100, 120, 130, 100, 130]], h, w).sum() == 0
    assert _poly_plane([[-50, -50, -20, -50, -20, -10]], h, w).sum() == 0
    # union = OR of the single encodings
    a = [3.2, 4.1, 25.7, 6.3, 20.2, 22.8, 6.6, 18.4]
    b = [15.5, 10.5, 38.2, 12.1, 30.9, 28.3]
    pa, pb = _poly_plane([a], h, w), _poly_plane([b], h, w)
    assert pa.sum() > 0 and pb.sum() > 0 and (pa & pb).sum() > 0
    np.testing.assert_array_equal(_poly_plane([a, b], h, w), pa | pb)
    np.testing.assert_array_equal(_poly_plane([b, a], h, w), pa | pb)
    # vertex order: reversed, rotated start
    pts = np.array(a).reshape(-1, 2)
    for k in range(4):
        rot = np.roll(pts, k, axis=0)
        np.testing.assert_array_equal(_poly_plane([rot.reshape(-1).tolist()], h, w), pa)
        np.testing.assert_array_equal(_poly_plane([rot[::-1].reshape(-1).tolist()], h, w), pa)
    # degenerate: valid RLEs
    for poly in ([], [5, 5], [5, 5, 20, 9], [5, 5, 5, 5, 5, 5], [2, 3, 12, 3, 22, 3]):
        _poly_plane([poly], h, w)
    assert _poly_plane([], h, w).sum() == 0
    # errors
    L = _mod("_lib").lib()
    n = C.c_int64(0)
    xy = np.array([0, 0, 10, 0, 10, 10, 0, 10], np.float64); offs = np.array([0, 4], np.int64)
    small = np.zeros(1, np.uint32)
    assert L.mrcnn_rle_from_polygons(xy.ctypes.data, offs.ctypes.data, 1, h, w, small.ctypes.data, 1, C.byref(n)) == 4 and n.value > 1
    assert L.mrcnn_rle_from_polygons(xy.ctypes.data, offs.ctypes.data, 1, 0, w, None, 0, C.byref(n)) == 4


def _center_sample(poly, h, w):
    """Even-odd rule at the pixel centres (x + .5, y + .5), float64."""
    pts = np.array(poly, np.float64).reshape(-1, 2)
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            px, py = x + 0.5, y + 0.5
            inside = False
            for i in range(len(pts)):
                (x1, y1), (x2, y2) = pts[i], pts[(i + 1) % len(pts)]
                if (y1 > py) != (y2 > py) and px < (x2 - x1) * (py - y1) / (y2 - y1) + x1:
                    inside = not inside
            out[y, x] = inside
    return out


def _dist_to_outline(poly, px, py):
    pts = np.array(poly, np.float64).reshape(-1, 2)
    best = math.inf
    for i in range(len(pts)):
        a, b = pts[i], pts[(i + 1) % len(pts)]
        ab = b - a
        t = 0.0 if not ab.any() else min(1.0, max(0.0, float(np.dot([px - a[0], py - a[1]], ab) / np.dot(ab, ab))))
        best = min(best, math.hypot(px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1])))
    return best


# How far the procedure can move the outline, in pixels (Euclidean), from its own steps:
#   a vertex is rounded to the 1/5 grid: <= 0.1 in x and in y                                  -> 0.1 * sqrt(2)
#   walking an edge, the minor coordinate of each fine point is rounded to the fine grid         -> 0.1
#   a fine point stands for the middle of its fine cell ((u + .5) / 5 - .5): half a cell in x, y -> 0.1 * sqrt(2)
#   a crossing takes the SMALLER fine row of the step across the column centre: one fine cell    -> 0.2
# A pixel whose centre is farther than that from the outline must agree with centre sampling.
BAND = 0.1 * math.sqrt(2) + 0.1 + 0.1 * math.sqrt(2) + 0.2


def test_polygons_against_center_sampling():
    rng = np.random.default_rng(3)
    h, w = 44, 52
    worst, differing, interior = 0.0, 0, 0
    for k in range(24):
        nv = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * math.pi, nv))
        rad = rng.uniform(6, 20, nv) if k % 2 else np.full(nv, rng.uniform(6, 20))     # star-shaped / convex (points of one circle)
        cx, cy = rng.uniform(12, w - 12), rng.uniform(12, h - 12)
        poly = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1).tolist()
        got, ref = _poly_plane([poly], h, w), _center_sample(poly, h, w)
        np.testing.assert_array_equal(ref != ref, np.zeros((h, w), bool))      # the sampling leg satisfies the condition trivially
        ys, xs = np.nonzero(got != ref)
        for y, x in zip(ys, xs):
            d = _dist_to_outline(poly, x + 0.5, y + 0.5)
            worst = max(worst, d)
            assert d <= BAND, f"polygon {k}: pixel ({x},{y}) differs {d:.3f} px from the outline (band {BAND:.3f})"
        differing += ys.size
        interior += int(ref.sum())
    print(f"centre sampling: {differing} boundary pixels differ over {interior} interior pixels, worst distance {worst:.3f} of {BAND:.3f}")
    assert interior > 3000


# ==================================================================================================================================
# COCOGroundTruth, accumulate / summarize, symbols
# ==================================================================================================================================
def test_ground_truth_reads_the_three_forms():
    CE, CR = _mod("coco_eval"), _mod("coco_results")
    h, w = 30, 41
    poly = [4, 5, 30, 5, 30, 21, 4, 21]
    plane = np.zeros((h, w), np.uint8); plane[5:21, 4:30] = 1
    r = CR.rle_encode(plane)
    forms = [[poly], {"size": [h, w], "counts": [int(v) for v in r["counts"]]}, {"size": [h, w], "counts": CR.rle_to_string(r["counts"])}]
    ds = {"images": [{"id": 9, "height": h, "width": w}], "categories": [{"id": 2}, {"id": 1}],
          "annotations": [{"id": i + 1, "image_id": 9, "category_id": 1, "iscrowd": int(i == 1), "area": 416.0, "bbox": [4, 5, 26, 16], "segmentation": s}
                          for i, s in enumerate(forms)]}
    gt = CE.COCOGroundTruth(ds)
    assert gt.cat_ids == [1, 2] and gt.img_ids() == [9] and gt.images[9] == (h, w)
    for a in gt.annotations:
        np.testing.assert_array_equal(gt.counts(a), r["counts"])
    assert [a["iscrowd"] for a in gt.annotations] == [0, 1, 0]
    import json, os, tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "a.json")
        with open(p, "w") as f:
            json.dump(ds, f)
        gt2 = CE.COCOGroundTruth(p)
        np.testing.assert_array_equal(gt2.counts(gt2.annotations[0]), r["counts"])
    with pytest.raises(ValueError):
        CE.segmentation_to_counts({"size": [h, w + 1], "counts": [int(v) for v in r["counts"]]}, h, w)


def _random_tables(rng, K=3, n_img=5):
    A, T = 4, 10
    E_np, E_naive = [], []
    for k in range(K):
        En, Ev = [], []
        for i in range(n_img):
            if k == 2 and i % 2:
                continue
            nd, ng = int(rng.integers(0, 14)), int(rng.integers(0, 5))
            scores = np.sort(rng.choice([0.9, 0.8, 0.7, 0.5, 0.5, 0.31], nd))[::-1].astype(np.float64)
            matched = rng.random((A, T, nd)) < 0.5
            ignore = rng.random((A, T, nd)) < 0.2
            gt_ig = rng.random((A, ng)) < (1.0 if k == 1 else 0.3)       # category 1: nothing to find in any range -> -1
            En.append({"scores": scores, "matched": matched, "ignore": ignore, "gt_ignore": gt_ig})
            Ev.append({"scores": scores.tolist(), "dtm": np.where(matched, 3, -1).tolist(), "dt_ig": ignore.astype(int).tolist(),
                       "gt_ig": gt_ig.astype(int).tolist()})
        E_np.append(En); E_naive.append(Ev)
    E_np.append([]); E_naive.append([])
    return E_np, E_naive


def test_accumulate_and_summarize_against_the_naive_leg():
    CE = _mod("coco_eval")
    thrs, rec = naive_thresholds()
    np.testing.assert_array_equal(thrs, CE.IOU_THRS); np.testing.assert_array_equal(rec, CE.REC_THRS)
    np.testing.assert_array_equal(np.array(N_AREA), CE.AREA_RNG)
    rng = np.random.default_rng(8)
    for _ in range(4):
        E_np, E_naive = _random_tables(rng)
        p, r = CE.accumulate(E_np)
        pn, rn = naive_accumulate(E_naive, len(thrs), rec)
        assert p.shape == (10, 101, 4, 4, 3) and r.shape == (10, 4, 4, 3)
        assert p.tobytes() == pn.tobytes() and r.tobytes() == rn.tobytes()
        stats, lines = CE.summarize(p, r)
        assert stats.tobytes() == naive_summarize(pn, rn, thrs).tobytes()
        assert len(lines) == 12 and lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {:0.3f}".format(stats[0])
        assert lines[1].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ]")
        assert lines[6].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ]")
        assert (p[:, :, 1] == -1).all() and (p[:, :, 3] == -1).all()


# (51 + 50 * 2/3) / 101 is the closed form WITHOUT COCOeval's np.spacing(1) in the precision's denominator; with it every one of the
# 101 points is smaller by at most one part in 2^52, and the mean of 101 doubles adds at most 101 roundings of 2^-53 relative:
# the procedure's value lies within (1 + 101) * 2^-52 of the closed form (the value itself is < 1).  Observed: 0.834983498349835.
KNOWN_AP = 0.8349834983498351
KNOWN_AP_TOL = 102 * 2.0 ** -52


def test_known_answer_tp_fp_tp_host():
    """One category, two objects, detections TP (0.9), FP (0.8), TP (0.7): AP = (51 + 50 * 2/3) / 101 at every threshold."""
    CE = _mod("coco_eval")
    A, T = 4, 10
    matched = np.broadcast_to(np.array([True, False, True]), (A, T, 3)).copy()
    e = {"scores": np.array([0.9, 0.8, 0.7]), "matched": matched, "ignore": np.zeros((A, T, 3), bool), "gt_ignore": np.zeros((A, 2), bool)}
    p, r = CE.accumulate([[e]])
    for t in range(T):
        ap = float(np.mean(p[t, :, 0, 0, 2].copy()))
        assert abs(ap - KNOWN_AP) <= KNOWN_AP_TOL, (t, repr(ap))
    assert np.all(r[:, 0, 0, 2] == 1.0) and np.all(r[:, 0, 0, 0] == 0.5)


def test_symbols_exported():
    lib_mod = _mod("_lib")
    L = lib_mod.lib()
    for s in ("mrcnn_rle_iou", "mrcnn_box_iou_xywh", "mrcnn_coco_match", "mrcnn_rle_from_polygons"):
        assert s in lib_mod.EXPORTED_SYMBOLS and hasattr(L, s)
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maskrcnn_hip.h")).read()
    for s in ("mrcnn_rle_iou(", "mrcnn_box_iou_xywh(", "mrcnn_coco_match(", "mrcnn_rle_from_polygons(", "mrcnn_iou_group", "mrcnn_match_group"):
        assert s in header
    assert C.sizeof(lib_mod.IouGroup) == 40 and C.sizeof(lib_mod.MatchGroup) == 32


def test_naive_leg_on_its_own_known_answers():
    """The yardstick must itself give the answers that need none: detections = ground truth -> 1.0 / -1, wrong category -> 0."""
    ds, _ = synthetic_dataset(SMALL_SIZES[:3], seed=2)
    ds["annotations"] = [a for a in ds["annotations"] if a["area"] > 0]
    for a in ds["annotations"]:
        a["iscrowd"] = 0
    CR = _mod("coco_results")
    res = [{"image_id": a["image_id"], "category_id": a["category_id"], "score": 0.9 - 0.001 * i, "bbox": a["bbox"],
            "segmentation": {"size": a["segmentation"]["size"], "counts": CR.rle_to_string(np.array(a["segmentation"]["counts"], np.uint32))}}
           for i, a in enumerate(ds["annotations"])]
    out = naive_score(ds, res, "segm")
    assert out["stats"][0] == 1.0 and out["stats"][8] == 1.0
    wrong = [dict(r, category_id=4) for r in res]
    assert naive_score(ds, wrong, "segm")["stats"][0] == 0.0
