"""COCOeval.accumulate on the GPU (mrcnn_coco_accumulate, coco_eval.accumulate_device, score(..., accumulate_on=...)).  The numpy
``coco_eval.accumulate`` is the definition: every comparison is np.array_equal on float64 against it, on the same records, through host
arrays (the library stages them) and through torch device tensors (read in place)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_coco_accumulate_host import random_evals
from test_coco_eval_host import SMALL_SIZES, synthetic_dataset

pytestmark = pytest.mark.gpu

SPACES = ["host", "device"]
GUARD = -77.25


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _both(evals, space, max_dets=(1, 10, 100), n_thrs=10, n_areas=4, rec_thrs=None):
    """(precision, recall) of the device entry and of numpy's accumulate, after asserting that they are equal."""
    CE = _mod("coco_eval")
    rec_thrs = CE.REC_THRS if rec_thrs is None else rec_thrs
    got = CE.accumulate_device(evals, max_dets, n_thrs, n_areas, rec_thrs, device=None if space == "host" else "cuda")
    want = CE.accumulate(evals, max_dets, n_thrs, n_areas, rec_thrs)
    for g, w, name in zip(got, want, ("precision", "recall")):
        assert g.dtype == np.float64 and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, int((g != w).sum()), g.size)
    return got


@pytest.mark.parametrize("space", SPACES)
def test_random_records_with_ties_everywhere(space):
    evals = random_evals(np.random.default_rng(7), K=5, n_img=60, max_nd=14)
    scores = np.concatenate([e["scores"] for e in evals[0]])
    assert scores.size > 300 and np.unique(scores).size <= 17                     # ties decide the order
    p, r = _both(evals, space)
    assert p.shape == (10, 101, 5, 4, 3) and (p[:, :, 4] == -1).all() and (r[:, 4] == -1).all() and (p[:, :, :4] > 0).any()
    _both(random_evals(np.random.default_rng(8), K=5, n_img=60, max_nd=6), space, max_dets=(1, 2, 5))


@pytest.fixture(scope="module")
def long_category():
    """Category 0: 95 images of 100 detections with 12 distinct scores; category 1: one entry; category 2: ground truth, no entry."""
    rng = np.random.default_rng(21)
    A, T = 4, 10
    E = []
    for i in range(95):
        scores = np.sort(rng.integers(1, 13, 100).astype(np.float32) / 16)[::-1].astype(np.float64)
        E.append({"scores": scores, "matched": rng.random((A, T, 100)) < 0.4, "ignore": rng.random((A, T, 100)) < 0.1, "gt_ignore": rng.random((A, 30)) < 0.3})
    one = {"scores": np.array([0.5]), "matched": np.ones((A, T, 1), bool), "ignore": np.zeros((A, T, 1), bool), "gt_ignore": np.zeros((A, 2), bool)}
    none = {"scores": np.zeros(0), "matched": np.zeros((A, T, 0), bool), "ignore": np.zeros((A, T, 0), bool), "gt_ignore": np.zeros((A, 3), bool)}
    evals = [E, [one], [none]]
    CE = _mod("coco_eval")
    return evals, CE.accumulate(evals)


@pytest.mark.parametrize("space", SPACES)
def test_a_category_spanning_many_chunks(space, long_category):
    CE = _mod("coco_eval")
    evals, want = long_category
    P = CE.pack_evals(evals)
    assert P["cat_offsets"].tolist() == [0, 9500, 9501, 9501]
    assert 9500 > 9 * CE.ACC_CHUNK                                                 # the segment spans ten sort and scan chunks
    s = np.sort(P["scores"][:9500])[::-1]
    assert s[4095] == s[4096] and s[8191] == s[8192]                               # ties straddle the merge boundaries
    got = CE.accumulate_device(evals, device=None if space == "host" else "cuda")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0][:, :, 2] == 0).all() and (got[1][:, 2] == 0).all() and (got[1][:, 1] == 0.5).all()


def _rec(scores, matched, ignore, gt_ignore, A=4, T=10):
    """A record whose flags are the same in every area range and threshold, unless given in full."""
    nd = len(scores)
    full = lambda f: np.broadcast_to(np.asarray(f, bool), (A, T, nd)).copy()
    g = np.asarray(gt_ignore, bool)
    return {"scores": np.asarray(scores, np.float64), "matched": full(matched), "ignore": full(ignore),
            "gt_ignore": g if g.ndim == 2 else np.broadcast_to(g, (A, g.size)).copy()}


@pytest.mark.parametrize("space", SPACES)
def test_edge_cells(space):
    CE = _mod("coco_eval")
    A, T, eps = 4, 10, np.spacing(1)
    assert CE.REC_THRS[50] == 0.5
    one_range = np.zeros((A, 2), bool); one_range[1] = True
    evals = [
        [_rec([], [], [], [0, 0])],                                                          # 0: ground truth, no detection
        [_rec([.9, .8], [1, 0], [0, 0], [1, 1, 1])],                                         # 1: detections, nothing to find in any range
        [_rec([.9, .8], [1, 0], [0, 0], one_range)],                                         # 2: nothing to find in range 1 only
        [_rec([.9, .8, .7], [1, 0, 1], [1, 1, 1], [0, 0])],                                  # 3: every entry ignored
        [_rec([.9, .5, .2], [1, 1, 0], [0, 0, 0], [0, 0]), _rec([.8, .6, .1], [0, 0, 0], [0, 0, 0], [0, 0])],    # 4: TP FP FP TP FP FP of 4
        [_rec([0.0, -0.0], [1, 0], [0, 0], [0, 0]), _rec([-0.0, 0.0, np.nan], [0, 1, 1], [0, 0, 0], [0])],       # 5: the zeros and a NaN
    ]
    p, r = _both(evals, space, max_dets=(1, 2, 3))
    assert (p[:, :, 0] == 0).all() and (r[:, 0] == 0).all()
    assert (p[:, :, 1] == -1).all() and (r[:, 1] == -1).all()
    assert (p[:, :, 2, 1] == -1).all() and (r[:, 2, 1] == -1).all() and (p[:, :, 2, 0] >= 0).all() and (r[:, 2, 0] == 0.5).all()
    assert (p[:, :, 3] == 0).all() and (r[:, 3] == 0).all()
    # category 4 under max_dets = 3: rc = .25 .25 .25 .5 .5 .5, pr = 1, 1/2, 1/3, 2/4, 2/5, 2/6 -> the envelope lifts 1/3 to 2/4
    q = p[0, :, 4, 0, 2]
    assert (r[:, 4, :, 2] == 0.5).all()
    assert (q[:26] == 1.0 / (1.0 + eps)).all() and (q[26:51] == 2.0 / (4.0 + eps)).all() and (q[51:] == 0).all()          # rc == REC_THRS[50]: >=
    # under max_dets = 1 only the two first entries take part: TP (.9), FP (.8)
    assert (p[0, :26, 4, 0, 0] == 1.0 / (1.0 + eps)).all() and (p[0, 26:, 4, 0, 0] == 0).all() and (r[:, 4, :, 0] == 0.25).all()
    # category 5: the order is 0.0 -0.0 | -0.0 0.0 by position (all equal), the NaN last: TP FP FP TP TP of 3
    assert (r[:, 5, :, 2] == 1.0).all() and (p[0, :34, 5, 0, 2] == 1.0 / (1.0 + eps)).all() and (p[0, 67:, 5, 0, 2] == 3.0 / (5.0 + eps)).all()


def test_argument_variations():
    CE = _mod("coco_eval")
    A, T = 4, 10
    none = lambda ng: {"scores": np.zeros(0), "matched": np.zeros((A, T, 0), bool), "ignore": np.zeros((A, T, 0), bool), "gt_ignore": np.zeros((A, ng), bool)}
    for space in SPACES:
        p, r = _both([[none(2)], [], [none(0)]], space)                           # n_dt = 0, K = 3
        assert (p[:, :, 0] == 0).all() and (p[:, :, 1:] == -1).all() and (r[:, 0] == 0).all()
        _both([], space)                                                            # K = 0
    evals = random_evals(np.random.default_rng(3), K=3, n_img=9)
    p, r = _both(evals, "host", rec_thrs=np.array([0.5]))
    assert p.shape == (10, 1, 3, 4, 3)
    _both(evals, "host", rec_thrs=np.array([-1.0, 0.0, 0.0, 0.3, 0.3, 1.0, 2.0]))
    small = random_evals(np.random.default_rng(4), K=3, A=1, T=1, n_img=9)
    p, r = _both(small, "device", n_thrs=1, n_areas=1)
    assert p.shape == (1, 101, 3, 1, 3) and r.shape == (1, 3, 1, 3)
    _both(evals, "device", max_dets=(100,))


@pytest.mark.parametrize("iou_type", ["segm", "bbox"])
def test_score_is_the_same_wherever_accumulate_runs(iou_type):
    CE = _mod("coco_eval")
    ds, res = synthetic_dataset(SMALL_SIZES, seed=5)
    gt = CE.COCOGroundTruth(ds)
    host = CE.score(gt, res, iou_type, accumulate_on="host")
    dev = CE.score(gt, res, iou_type, accumulate_on="device")
    resident = CE.score(gt, res, iou_type, device_gt=gt.to_device(), accumulate_on="device")
    default = CE.score(gt, res, iou_type)
    for k in ("precision", "recall", "stats"):
        assert np.array_equal(host[k], dev[k]) and np.array_equal(host[k], resident[k]) and np.array_equal(host[k], default[k]), k
    assert host["summary"] == dev["summary"] and 0.0 < host["stats"][0] < 1.0


def test_score_batch_with_resident_ground_truth():
    """Detections left on the device, ground truth resident there: score_batch gives the same arrays with either accumulate."""
    import torch
    CE, CR, D, E = _mod("coco_eval"), _mod("coco_results"), _mod("detection"), _mod("evaluate")
    rng = np.random.default_rng(31)
    sizes = [(240, 320), (130, 120)]
    H, W, rows = 256, 320, 12
    B = len(sizes)
    det = np.zeros((B, rows, 6), np.float32)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    masks = np.zeros((B, rows, 28, 28), np.float32)
    for b, (h, w) in enumerate(sizes):
        nh, nw, py, px = E.letterbox_geometry(h, w, H, W)
        for i in range(rows - 2):
            y1 = (py + rng.uniform(0, 0.6) * nh) / (H - 1); x1 = (px + rng.uniform(0, 0.6) * nw) / (W - 1)
            det[b, i] = [y1, x1, min(1.0, y1 + rng.uniform(0.05, 0.4) * nh / H), min(1.0, x1 + rng.uniform(0.05, 0.4) * nw / W), rng.integers(1, 3),
                         0.3 + 0.6 * rng.random()]
            cy, cx, sy, sx = rng.uniform(8, 20), rng.uniform(8, 20), rng.uniform(4, 12), rng.uniform(4, 12)
            masks[b, i] = np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
    image_ids = [20, 10]
    det_src, rles, areas, _ = D.masks_rle_source(det, masks, sizes, H, W, 0.5)
    results = CR.coco_results(image_ids, det_src, rles, sizes)
    anns = []
    for k, res in enumerate(results[::2]):
        plane = CR.rle_decode(res["segmentation"])
        if k % 3 == 1:
            plane = np.roll(plane, 4, 1)
        if plane.sum() == 0:
            continue
        anns.append({"id": k + 1, "image_id": res["image_id"], "category_id": res["category_id"], "iscrowd": 0, "area": float(plane.sum()),
                     "bbox": list(res["bbox"]), "segmentation": {"size": list(plane.shape), "counts": CR.rle_to_string(CR.rle_encode(plane)["counts"])}})
    assert len(anns) > 5
    ds = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(image_ids, sizes)], "categories": [{"id": c} for c in (1, 2)], "annotations": anns}
    gt = CE.COCOGroundTruth(ds)
    batches = [CE.device_detections(image_ids, torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, H, W, 0.5)]
    resident = gt.to_device()
    for iou_type in ("segm", "bbox"):
        host = CE.score_batch(gt, batches, iou_type, device_gt=resident, accumulate_on="host")
        dev = CE.score_batch(gt, batches, iou_type, device_gt=resident, accumulate_on="device")
        for k in ("precision", "recall", "stats"):
            assert np.array_equal(host[k], dev[k]), (iou_type, k)
        assert host["stats"][0] > 0.0


@pytest.mark.parametrize("space", SPACES)
def test_guards_around_the_outputs_stay_and_nothing_between_survives(space):
    CE, lib_mod = _mod("coco_eval"), _mod("_lib")
    L = lib_mod.lib()
    evals = random_evals(np.random.default_rng(12), K=4, n_img=7)
    P = CE.pack_evals(evals)
    A, T, n = P["matched"].shape
    K, M, R, G = 4, 3, CE.REC_THRS.size, 64
    md, thr = np.array([1, 10, 100], np.int32), np.ascontiguousarray(CE.REC_THRS)
    n_p, n_r = T * R * K * A * M, T * K * A * M
    if space == "host":
        pbuf, rbuf = np.full(n_p + 2 * G, GUARD), np.full(n_r + 2 * G, GUARD)
        tabs = [P["scores"], P["ranks"], P["matched"], P["ignore"]]
        ptr, at = (lambda a: a.ctypes.data), (lambda a: a.ctypes.data + 8 * G)
        memspace = lib_mod.HOST
    else:
        import torch
        pbuf = torch.full((n_p + 2 * G,), GUARD, dtype=torch.float64, device="cuda")
        rbuf = torch.full((n_r + 2 * G,), GUARD, dtype=torch.float64, device="cuda")
        tabs = [torch.from_numpy(P[k]).cuda() for k in ("scores", "ranks", "matched", "ignore")]
        ptr, at = (lambda a: a.data_ptr()), (lambda a: a.data_ptr() + 8 * G)
        memspace = lib_mod.DEVICE
    lib_mod.check(L.mrcnn_coco_accumulate(ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), n, P["cat_offsets"].ctypes.data, K,
                                          P["npig"].ctypes.data, A, T, md.ctypes.data, M, thr.ctypes.data, R, memspace, at(pbuf), at(rbuf)))
    if space == "device":
        pbuf, rbuf = pbuf.cpu().numpy(), rbuf.cpu().numpy()
    want = CE.accumulate(evals)
    for buf, size, w in ((pbuf, n_p, want[0]), (rbuf, n_r, want[1])):
        assert (buf[:G] == GUARD).all() and (buf[G + size:] == GUARD).all()
        assert not (buf[G:G + size] == GUARD).any()
        assert np.array_equal(buf[G:G + size].reshape(w.shape), w)
