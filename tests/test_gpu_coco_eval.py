"""COCO scoring on the GPU (mrcnn_rle_iou, mrcnn_box_iou_xywh, mrcnn_coco_match, coco_eval.score, evaluate.evaluate_coco_scored)
against the naive restatement of COCO's procedure in tests/test_coco_eval_host.py (dense planes, Python loops).  Every comparison
is exact: intersections as integers, IoUs / precision / recall / stats bit for bit."""
import ctypes as C
import importlib
import json

import numpy as np
import pytest

from test_coco_eval_host import (KNOWN_AP, KNOWN_AP_TOL, N_AREA, SMALL_SIZES, ellipse, naive_box_iou, naive_evaluate_img, naive_mask_iou,
                                 naive_score, naive_thresholds, synthetic_dataset, tight_box)

pytestmark = pytest.mark.gpu

MIXED_SIZES = [(480, 640), (427, 640), (640, 480), (375, 500), (333, 500), (500, 375), (240, 320), (612, 612)]   # tools/mixed_batch_ab.py
GUARD_U32, GUARD_F64 = 0x5A5A5A5A, -77.25


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _rle_set(planes):
    CR = _mod("coco_results")
    rles = [CR.rle_encode(p)["counts"] for p in planes]
    offs = np.zeros(len(rles) + 1, np.int64)
    offs[1:] = np.cumsum([r.size for r in rles])
    return np.ascontiguousarray(np.concatenate(rles), dtype=np.uint32), offs


def _groups(table):
    lib = _mod("_lib")
    arr = (lib.IouGroup * max(1, len(table)))()
    for k, g in enumerate(table):
        arr[k].d0, arr[k].d1, arr[k].g0, arr[k].g1, arr[k].out_offset = g
    return arr


def _call_rle_iou(space, dc, do, gc, go, crowd, table, n_pairs, inter, iou):
    """Through the C ABI in either memspace; inter / iou are host arrays that arrive pre-filled (guard values) and come back."""
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    nd, ng = do.size - 1, go.size - 1
    if space == "host":
        return L.mrcnn_rle_iou(dc.ctypes.data, do.ctypes.data, nd, gc.ctypes.data, go.ctypes.data, ng, crowd.ctypes.data, _groups(table), len(table),
                               lib.HOST, inter.ctypes.data, iou.ctypes.data, n_pairs)
    t = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in (dc, do, gc, go, inter, iou)]
    st = L.mrcnn_rle_iou(t[0].data_ptr(), t[1].data_ptr(), nd, t[2].data_ptr(), t[3].data_ptr(), ng, crowd.ctypes.data, _groups(table), len(table),
                         lib.DEVICE, t[4].data_ptr(), t[5].data_ptr(), n_pairs)
    inter[:] = t[4].cpu().numpy().view(np.uint32)
    iou[:] = t[5].cpu().numpy()
    return st


def _special_planes(h, w, rng):
    noise = (rng.random((h, w)) < 0.5).astype(np.uint8)                     # thousands of runs: beyond what a block stages in LDS
    stripes = np.zeros((h, w), np.uint8); stripes[h // 4: h // 2, :] = 1       # one run of ones per column
    single = np.zeros((h, w), np.uint8); single[h // 3, w // 5] = 1
    first = np.zeros((h, w), np.uint8); first[0, 0] = 1; first[h - 1, w - 1] = 1      # counts[0] = 0, and a last run of ones
    blob = ellipse(h, w, h * 0.4, w * 0.6, h * 0.3, w * 0.25)
    return [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), single, stripes, noise, first, blob,
            (blob & noise).astype(np.uint8), np.roll(blob, 3, 1), ellipse(h, w, h * 0.5, w * 0.5, h * 0.1, w * 0.45)]


@pytest.mark.parametrize("space", ["device", "host"])
def test_rle_iou_is_exact_for_every_pair(space):
    rng = np.random.default_rng(17)
    d_planes, g_planes, table, crowd = [], [], [], []
    out_at = 7                                                               # the first block does not start at 0: a gap nobody writes
    for (h, w) in [(60, 83), (128, 96), (1, 50), (97, 1), (200, 140)]:
        sp = _special_planes(h, w, rng)
        ds = sp + [np.roll(sp[6], -2, 0)]
        gs = sp[::-1][:9]
        d0, g0 = len(d_planes), len(g_planes)
        d_planes += ds; g_planes += gs
        crowd += [int(j % 4 == 1) for j in range(len(gs))]
        table.append((d0, d0 + len(ds), g0, g0 + len(gs), out_at))
        out_at += len(ds) * len(gs) + 3
    table.append((2, 2, 0, 3, out_at))                                        # a group without detections, one without ground truth
    table.append((0, 3, 4, 4, out_at))
    n_pairs = out_at + 5
    dc, do = _rle_set(d_planes); gc, go = _rle_set(g_planes)
    assert max(np.diff(go)) > 4096 and max(np.diff(do)) > 4096                # the noise masks
    crowd = np.array(crowd, np.uint8)
    inter = np.full(n_pairs, GUARD_U32, np.uint32); iou = np.full(n_pairs, GUARD_F64, np.float64)
    st = _call_rle_iou(space, dc, do, gc, go, crowd, table, n_pairs, inter, iou)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    covered = np.zeros(n_pairs, bool)
    checked = 0
    for (d0, d1, g0, g1, off) in table:
        if d1 == d0 or g1 == g0:
            continue
        want_inter, want_iou = naive_mask_iou(d_planes[d0:d1], g_planes[g0:g1], crowd[g0:g1])
        ng = g1 - g0
        for i in range(d1 - d0):
            for j in range(ng):
                o = off + i * ng + j
                covered[o] = True
                assert int(inter[o]) == want_inter[i][j], (space, d0 + i, g0 + j)
                assert iou[o].tobytes() == np.float64(want_iou[i, j]).tobytes(), (space, d0 + i, g0 + j, iou[o], want_iou[i, j])
                checked += 1
    assert checked > 400
    assert np.all(inter[~covered] == GUARD_U32) and np.all(iou[~covered] == GUARD_F64)     # entries no block covers stay untouched


@pytest.mark.parametrize("space", ["device", "host"])
def test_rle_iou_refuses_unequal_planes_and_bad_tables(space):
    lib = _mod("_lib")
    a = [np.ones((10, 12), np.uint8), ellipse(10, 12, 5, 5, 3, 3)]
    b = [ellipse(10, 12, 4, 6, 3, 4), np.ones((10, 13), np.uint8)]            # the second ground truth is a plane of another size
    dc, do = _rle_set(a); gc, go = _rle_set(b)
    crowd = np.zeros(2, np.uint8)
    inter = np.full(4, GUARD_U32, np.uint32); iou = np.full(4, GUARD_F64, np.float64)
    assert _call_rle_iou(space, dc, do, gc, go, crowd, [(0, 2, 0, 2, 0)], 4, inter, iou) == 4          # MRCNN_ERR_SHAPE
    assert b"pixels" in lib.lib().mrcnn_last_error()
    assert np.all(inter == GUARD_U32) and np.all(iou == GUARD_F64)
    assert _call_rle_iou(space, dc, do, gc, go, crowd, [(0, 2, 0, 1, 0)], 4, inter, iou) == 0          # the consistent part alone is fine
    assert np.all(inter[2:] == GUARD_U32) and int(inter[0]) == int(b[0].sum())
    for bad in ([(0, 3, 0, 1, 0)], [(0, 2, 0, 1, 3)], [(0, 2, 0, 1, -1)], [(0, 1, 0, 1, 0), (1, 2, 0, 1, 0)]):
        assert _call_rle_iou(space, dc, do, gc, go, crowd, bad, 4, inter, iou) == 4, bad


@pytest.mark.parametrize("space", ["device", "host"])
def test_box_iou_xywh(space):
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    rng = np.random.default_rng(4)
    db = np.concatenate([rng.uniform(0, 50, (40, 2)), rng.uniform(0.5, 60, (40, 2))], 1)
    gb = np.concatenate([rng.uniform(0, 50, (9, 2)), rng.uniform(0.5, 60, (9, 2))], 1)
    gb[0] = [3, 4, 20, 10]; db[0] = gb[0]; db[1] = [0, 0, 0, 0]; gb[1] = [0, 0, 0, 0]; db[2] = [10, 10, 5, 5]; gb[2] = [15, 10, 5, 5]     # equal, empty, touching
    crowd = np.array([0, 0, 0, 1, 0, 1, 0, 0, 0], np.uint8)
    table = [(0, 25, 0, 4, 2), (25, 40, 4, 9, 2 + 100)]
    n_pairs = 2 + 100 + 75 + 1
    iou = np.full(n_pairs, GUARD_F64, np.float64)
    if space == "host":
        st = L.mrcnn_box_iou_xywh(db.ctypes.data, 40, gb.ctypes.data, 9, crowd.ctypes.data, _groups(table), 2, lib.HOST, iou.ctypes.data, n_pairs)
    else:
        t = [torch.from_numpy(a).cuda() for a in (db, gb, iou)]
        st = L.mrcnn_box_iou_xywh(t[0].data_ptr(), 40, t[1].data_ptr(), 9, crowd.ctypes.data, _groups(table), 2, lib.DEVICE, t[2].data_ptr(), n_pairs)
        iou = t[2].cpu().numpy()
    assert st == 0
    for (d0, d1, g0, g1, off) in table:
        want = naive_box_iou(db[d0:d1], gb[g0:g1], crowd[g0:g1])
        got = iou[off:off + want.size].reshape(want.shape)
        assert got.tobytes() == want.tobytes()
    assert iou[0] == GUARD_F64 and iou[1] == GUARD_F64 and iou[-1] == GUARD_F64
    assert iou[2] == 1.0


def _match_through_abi(space, dataset, results, iou_type="segm"):
    """mrcnn_rle_iou + mrcnn_coco_match driven by tables built HERE (not by coco_eval.py); returns {(image, category): (dt_match,
    dt_ignore, gt_match) as (A, T, n) arrays} with positions as the kernel documents them."""
    import torch
    lib, CR = _mod("_lib"), _mod("coco_results")
    L = lib.lib()
    thrs, _ = naive_thresholds()
    imgs = sorted(im["id"] for im in dataset["images"])
    d_planes, g_planes, table, crowd, at = [], [], [], [], 0
    img_info = {}
    for img in imgs:
        gts = [a for a in dataset["annotations"] if a["image_id"] == img]
        dts = [r for r in results if r["image_id"] == img]
        d0, g0 = len(d_planes), len(g_planes)
        d_planes += [CR.rle_decode(r["segmentation"]) for r in dts]
        g_planes += [CR.rle_decode(a["segmentation"]) for a in gts]
        crowd += [int(a["iscrowd"]) for a in gts]
        table.append((d0, d0 + len(dts), g0, g0 + len(gts), at))
        img_info[img] = (at, dts, gts)
        at += len(dts) * len(gts)
    n_pairs = at
    dc, do = _rle_set(d_planes); gc, go = _rle_set(g_planes)
    inter = np.zeros(n_pairs, np.uint32); iou = np.zeros(n_pairs, np.float64)
    assert _call_rle_iou(space, dc, do, gc, go, np.array(crowd, np.uint8), table, n_pairs, inter, iou) == 0
    groups, keys, dt_idx, dt_area, gt_idx, gt_area, gt_crowd = [], [], [], [], [], [], []
    for img in imgs:
        off, dts, gts = img_info[img]
        for cat in sorted(c["id"] for c in dataset["categories"]):
            di = [i for i, r in enumerate(dts) if r["category_id"] == cat]
            gi = [j for j, a in enumerate(gts) if a["category_id"] == cat]
            if not di and not gi:
                continue
            di = [di[i] for i in sorted(range(len(di)), key=lambda i: -dts[di[i]]["score"])][:100]
            a0, b0 = len(dt_idx), len(gt_idx)
            dt_idx += di; gt_idx += gi
            dt_area += [float(d_planes[table[imgs.index(img)][0] + i].sum()) for i in di]
            gt_area += [float(gts[j]["area"]) for j in gi]
            gt_crowd += [int(gts[j]["iscrowd"]) for j in gi]
            groups.append((off, len(gts), a0, len(dt_idx), b0, len(gt_idx)))
            keys.append((img, cat))
    marr = (lib.MatchGroup * len(groups))()
    for k, g in enumerate(groups):
        marr[k].iou_offset, marr[k].iou_stride, marr[k].dt0, marr[k].dt1, marr[k].gt0, marr[k].gt1 = g
    A, T = len(N_AREA), len(thrs)
    dt_idx = np.array(dt_idx, np.int32); dt_area = np.array(dt_area, np.float64)
    gt_idx = np.array(gt_idx, np.int32); gt_area = np.array(gt_area, np.float64); gt_crowd = np.array(gt_crowd, np.uint8)
    rng = np.array(N_AREA, np.float64); thr = np.ascontiguousarray(thrs, np.float64)
    dm = np.full(A * T * dt_idx.size, 99, np.int32); dg = np.full(A * T * dt_idx.size, 99, np.uint8); gm = np.full(A * T * gt_idx.size, 99, np.int32)
    args = [marr, len(groups), dt_idx.ctypes.data, dt_area.ctypes.data, dt_idx.size, gt_idx.ctypes.data, gt_area.ctypes.data, gt_crowd.ctypes.data, gt_idx.size,
            rng.ctypes.data, A, thr.ctypes.data, T]
    if space == "host":
        st = L.mrcnn_coco_match(iou.ctypes.data, n_pairs, lib.HOST, *args, dm.ctypes.data, dg.ctypes.data, gm.ctypes.data)
    else:
        t = [torch.from_numpy(a).cuda() for a in (iou, dm, dg, gm)]
        st = L.mrcnn_coco_match(t[0].data_ptr(), n_pairs, lib.DEVICE, *args, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr())
        dm, dg, gm = t[1].cpu().numpy(), t[2].cpu().numpy(), t[3].cpu().numpy()
    assert st == 0, L.mrcnn_last_error()
    out = {}
    for key, g in zip(keys, groups):
        nd, ng = g[3] - g[2], g[5] - g[4]
        out[key] = (dm[A * T * g[2]:A * T * g[3]].reshape(A, T, nd), dg[A * T * g[2]:A * T * g[3]].reshape(A, T, nd),
                    gm[A * T * g[4]:A * T * g[5]].reshape(A, T, ng))
    return out


@pytest.mark.parametrize("space", ["device", "host"])
def test_coco_match_equals_naive_evaluate_img(space):
    ds, res = synthetic_dataset(SMALL_SIZES, seed=5)
    got = _match_through_abi(space, ds, res)
    per = naive_score(ds, res, "segm")["per"]
    assert set(got) == set(per) and len(per) > 15
    matched = ignored = crowd_rematch = 0
    for key, e in per.items():
        dm, dg, gm = got[key]
        np.testing.assert_array_equal(dm, np.array(e["dtm"], np.int32).reshape(dm.shape), err_msg=str(key))
        np.testing.assert_array_equal(dg, np.array(e["dt_ig"], np.uint8).reshape(dg.shape), err_msg=str(key))
        np.testing.assert_array_equal(gm, np.array(e["gtm"], np.int32).reshape(gm.shape), err_msg=str(key))
        matched += int((dm >= 0).sum()); ignored += int(dg.sum())
    assert matched > 100 and ignored > 100                                       # the cases exist
    assert max(len(e["scores"]) for e in per.values()) == 100                    # the > 100 detections of one image were cut


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_score_equals_the_naive_leg(iou_type):
    CE = _mod("coco_eval")
    for compressed in (False, True):
        ds, res = synthetic_dataset(SMALL_SIZES, seed=5 + int(compressed), compressed=compressed)
        out = CE.score(CE.COCOGroundTruth(ds), res, iou_type)
        want = naive_score(ds, res, iou_type)
        assert out["precision"].shape == (10, 101, 5, 4, 3) and out["recall"].shape == (10, 5, 4, 3) and len(out["summary"]) == 12
        assert out["precision"].tobytes() == want["precision"].tobytes()
        assert out["recall"].tobytes() == want["recall"].tobytes()
        assert out["stats"].tobytes() == want["stats"].tobytes()
        assert 0.0 < out["stats"][0] < 1.0 and (out["precision"][:, :, 3] == -1).all()       # category 4 has no ground truth
        # a subset of the images
        sub = [im["id"] for im in ds["images"]][1:4]
        assert CE.score(CE.COCOGroundTruth(ds), res, iou_type, img_ids=sub)["precision"].tobytes() == naive_score(ds, res, iou_type, sub)["precision"].tobytes()


def test_score_on_the_mixed_sizes_smoke_of_full_planes():
    """The eight sizes of tools/mixed_batch_ab.py once, segm: full-resolution planes through the same comparison (fewer objects)."""
    CE = _mod("coco_eval")
    ds, res = synthetic_dataset(MIXED_SIZES[:3], seed=9)
    ds["annotations"] = [a for a in ds["annotations"] if a["id"] % 2]
    res = res[::3]
    out, want = CE.score(CE.COCOGroundTruth(ds), res, "segm"), naive_score(ds, res, "segm")
    assert out["precision"].tobytes() == want["precision"].tobytes() and out["stats"].tobytes() == want["stats"].tobytes()
    assert out["stats"][5] > -1                                                    # objects above 96^2 exist at this size


def _as_results(anns, score=lambda i: 0.9 - 1e-3 * i):
    CR = _mod("coco_results")
    out = []
    for i, a in enumerate(anns):
        c = a["segmentation"]["counts"]
        out.append({"image_id": a["image_id"], "category_id": a["category_id"], "score": float(score(i)), "bbox": list(a["bbox"]),
                    "segmentation": {"size": a["segmentation"]["size"], "counts": c if isinstance(c, str) else CR.rle_to_string(np.array(c, np.uint32))}})
    return out


def test_known_answers():
    CE, CR = _mod("coco_eval"), _mod("coco_results")
    ds, _ = synthetic_dataset(SMALL_SIZES, seed=12)
    ds["annotations"] = [a for a in ds["annotations"] if a["area"] > 0 and not a["iscrowd"]]
    gt = CE.COCOGroundTruth(ds)
    res = _as_results(ds["annotations"])
    for iou_type in ("segm", "bbox"):
        out = CE.score(gt, res, iou_type)
        s = out["stats"]
        assert s[0] == 1.0 and s[1] == 1.0 and s[2] == 1.0 and s[8] == 1.0, (iou_type, s)
        areas = np.array([a["area"] for a in ds["annotations"]])
        for k, (lo, hi) in enumerate(N_AREA[1:]):
            present = bool(((areas >= lo) & (areas <= hi)).any())
            assert s[3 + k] == (1.0 if present else -1.0) and s[9 + k] == (1.0 if present else -1.0), (iou_type, k, s)
        for k, cat in enumerate(out["cat_ids"]):
            has = any(a["category_id"] == cat for a in ds["annotations"])
            pk = out["precision"][:, :, k, 0, 2]
            assert (pk == -1).all() if not has else (pk > 0.999999).all()
        # all detections in the wrong category -> 0; no detections at all -> 0
        assert CE.score(gt, [dict(r, category_id=4) for r in res], iou_type)["stats"][0] == 0.0
        none = CE.score(gt, [], iou_type)["stats"]
        assert none[0] == 0.0 and none[8] == 0.0
    # one category, one image, two objects, TP (0.9), FP (0.8), TP (0.7) at IoU 1
    h, w = 40, 50
    a, b, fp = ellipse(h, w, 10, 12, 6, 8), ellipse(h, w, 28, 35, 8, 9), ellipse(h, w, 33, 8, 4, 4)
    assert (a & fp).sum() == 0 and (b & fp).sum() == 0
    anns = [{"id": i + 1, "image_id": 1, "category_id": 7, "iscrowd": 0, "area": float(p.sum()), "bbox": tight_box(p),
             "segmentation": {"size": [h, w], "counts": [int(v) for v in CR.rle_encode(p)["counts"]]}} for i, p in enumerate((a, b))]
    fp_ann = dict(anns[0], bbox=tight_box(fp), segmentation={"size": [h, w], "counts": [int(v) for v in CR.rle_encode(fp)["counts"]]})
    ds2 = {"images": [{"id": 1, "height": h, "width": w}], "categories": [{"id": 7}], "annotations": anns}
    res2 = _as_results([anns[0], fp_ann, anns[1]], score=lambda i: [0.9, 0.8, 0.7][i])
    for iou_type in ("segm", "bbox"):
        out = CE.score(CE.COCOGroundTruth(ds2), res2, iou_type)
        for t in range(10):
            ap = float(np.mean(out["precision"][t, :, 0, 0, 2].copy()))
            print(iou_type, t, repr(ap))
            assert abs(ap - KNOWN_AP) <= KNOWN_AP_TOL, (iou_type, t, repr(ap))          # the bound: see tests/test_coco_eval_host.py
        assert out["stats"][8] == 1.0 and out["stats"][6] == 0.5


def test_invariances():
    CE = _mod("coco_eval")
    ds, res = synthetic_dataset(SMALL_SIZES, seed=21)
    # unequal scores everywhere: the order among equal scores is the one thing the procedure leaves to the input order
    rng = np.random.default_rng(1)
    for i, r in enumerate(res):
        r["score"] = float(0.05 + 0.9 * (i + 1) / (len(res) + 1))
    base = {t: CE.score(CE.COCOGroundTruth(ds), res, t) for t in ("segm", "bbox")}

    def same(ds2, res2):
        for t in ("segm", "bbox"):
            o = CE.score(CE.COCOGroundTruth(ds2), res2, t)
            for k in ("precision", "recall", "stats"):
                assert o[k].tobytes() == base[t][k].tobytes(), (t, k)
    same(ds, [res[i] for i in rng.permutation(len(res))])
    same(dict(ds, images=[ds["images"][i] for i in rng.permutation(len(ds["images"]))]), res)
    same(dict(ds, annotations=[ds["annotations"][i] for i in rng.permutation(len(ds["annotations"]))]), res)
    same(json.loads(json.dumps(ds)), json.loads(json.dumps(res)))               # the list loaded from JSON


def test_device_fast_path_equals_the_path_through_strings():
    """Detections left on the device by mrcnn_masks_rle_source (read in place) against the same detections through coco_results'
    compressed strings; ground truth = some of the detections' own masks, some shifted, one crowd."""
    import torch
    CE, CR, D, E = _mod("coco_eval"), _mod("coco_results"), _mod("detection"), _mod("evaluate")
    rng = np.random.default_rng(31)
    sizes = MIXED_SIZES[:4]
    H, W, rows = 256, 320, 20
    B = len(sizes)
    det = np.zeros((B, rows, 6), np.float32)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    masks = np.zeros((B, rows, 28, 28), np.float32)
    for b, (h, w) in enumerate(sizes):
        nh, nw, py, px = E.letterbox_geometry(h, w, H, W)
        for i in range(rows - 3):                                                  # the last rows stay padding
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
        plane = CR.rle_decode(r["segmentation"])
        if k % 3 == 1:
            plane = np.roll(plane, 4, 1)
        if plane.sum() == 0:
            continue
        anns.append({"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": int(k % 7 == 3), "area": float(plane.sum()),
                     "bbox": [r["bbox"][0] + (4.0 if k % 3 == 1 else 0.0)] + r["bbox"][1:],     # the detection's own box (shifted like the mask), not the mask's
                     "segmentation": {"size": list(plane.shape), "counts": CR.rle_to_string(CR.rle_encode(plane)["counts"])}})
    ds = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(image_ids, sizes)], "categories": [{"id": c} for c in (1, 2, 3)], "annotations": anns}
    assert len(anns) > 20
    gt = CE.COCOGroundTruth(ds)
    # two device batches of two images
    batches = [CE.device_detections(image_ids[s:s + 2], torch.from_numpy(det[s:s + 2]).cuda(), torch.from_numpy(masks[s:s + 2]).cuda(), sizes[s:s + 2], H, W, 0.5)
               for s in (0, 2)]
    assert all(b.counts.is_cuda and b.run_offsets.is_cuda for b in batches)
    for iou_type in ("segm", "bbox"):
        a = CE.score(gt, results, iou_type)
        b = CE.score_batch(gt, batches, iou_type)
        want = naive_score(ds, results, iou_type)
        for k in ("precision", "recall", "stats"):
            assert a[k].tobytes() == b[k].tobytes() == want[k].tobytes(), (iou_type, k)
        assert 0.0 < a["stats"][0] <= 1.0


@pytest.mark.parametrize("mode", ["f32x3", "f16"])
def test_evaluate_coco_scored_end_to_end(pkg, small_model, mode, tmp_path):
    """The model's own detections of a first run fed back as ground truth (RLE annotations): AP = 1 for segm and bbox; with half of
    the annotations removed the naive leg's value."""
    CE, CR, E = _mod("coco_eval"), _mod("coco_results"), _mod("evaluate")
    d, cfg = small_model
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype=mode)
    sizes = [(96, 160), (300, 200), (128, 128), (37, 53), (64, 427), (333, 100), (200, 201)]          # tests/test_gpu_rle.py's seven images
    rng = np.random.default_rng(11)
    pixels = {50 - i: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)}
    items = [(i, p) for i, p in pixels.items()]
    _, _, _, first = E.evaluate_segm(m, items, limit=None, verbose=False, batch=4)
    anns, teeth = [], 0
    for k, r in enumerate(first):
        plane = CR.rle_decode(r["segmentation"])
        if plane.sum() == 0:                                                         # IoU 0 / 0 = 0 with itself: can match nothing
            continue
        teeth += int(0 < int(plane.sum()) < plane.size)
        anns.append({"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "area": float(plane.sum()), "bbox": r["bbox"],
                     "segmentation": {"size": r["segmentation"]["size"], "counts": r["segmentation"]["counts"]}})
    assert teeth > 0, "no detection with a non-empty, non-full mask: the comparison has no teeth"
    cats = sorted(set(a["category_id"] for a in anns))

    def run(annotations, name):
        ds = {"images": [{"id": i, "height": p.shape[0], "width": p.shape[1], "file_name": f"{i}.png", "coco_url": "", "flickr_url": "",
                          "date_captured": "", "license": 0} for i, p in pixels.items()],
              "categories": [{"id": c, "name": str(c), "supercategory": ""} for c in cats], "annotations": annotations,
              "info": {}, "licenses": []}
        path = str(tmp_path / name)
        with open(path, "w") as f:
            json.dump(ds, f)
        out = E.evaluate_coco_scored(m, path, lambda im: pixels[im.id], limit=7, verbose=False, batch=4)
        assert len(out) == 5 and set(out[4]) == {"bbox", "segm"}
        return ds, out
    ds, out = run(anns, "all.json")
    results = out[3]
    scored = [r for r in results if CR.rle_decode(r["segmentation"]).sum() > 0]
    assert len(scored) == len(anns) > 0
    for iou_type in ("segm", "bbox"):
        s = out[4][iou_type]
        want = naive_score(ds, results, iou_type)
        for k in ("precision", "recall", "stats"):
            assert s[k].tobytes() == want[k].tobytes(), (mode, iou_type, k)
        if len(scored) == len(results):                                               # every detection fed back has a non-empty mask
            assert s["stats"][0] == 1.0 and s["stats"][8] == 1.0, (mode, iou_type, s["stats"])
        print(mode, iou_type, "AP", s["stats"][0], "detections", len(results), "annotations", len(anns))
    ds2, out2 = run(anns[::2], "half.json")
    for iou_type in ("segm", "bbox"):
        want = naive_score(ds2, out2[3], iou_type)
        assert out2[4][iou_type]["stats"].tobytes() == want["stats"].tobytes()
        assert out2[4][iou_type]["precision"].tobytes() == want["precision"].tobytes()
        print(mode, iou_type, "AP with half of the annotations", out2[4][iou_type]["stats"][0])
