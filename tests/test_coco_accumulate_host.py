"""mrcnn_coco_accumulate without a GPU: the entry is declared, bound and exported; every argument error is answered before the device is
touched (so the codes below do not depend on whether a device is present); ``pack_evals`` lays the per-image records out as the flat
tables of the entry — compared with the concatenations ``accumulate`` builds for itself."""
import importlib
import inspect
import os

import numpy as np
import pytest

INVALID, SHAPE = 1, 4


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maskrcnn_hip.h")).read()


def random_evals(rng, K=5, A=4, T=10, n_img=6, max_nd=14, quantum=16.0, gt_ignore_p=0.3):
    """evals[k] = per-image records as coco_eval.accumulate takes them: scores are float32 values quantised to 1 / quantum, descending
    inside a record, so ties are everywhere; matched / ignore / gt_ignore are random.  Category K - 1 has no record at all."""
    evals = []
    for k in range(K):
        E = []
        for i in range(n_img):
            if k == K - 1 or (k == 2 and i % 2):
                continue
            nd, ng = int(rng.integers(0, max_nd + 1)), int(rng.integers(0, 5))
            scores = np.sort(np.round(rng.random(nd).astype(np.float32) * quantum) / quantum)[::-1].astype(np.float64)
            E.append({"scores": scores, "matched": rng.random((A, T, nd)) < 0.5, "ignore": rng.random((A, T, nd)) < 0.2,
                      "gt_ignore": rng.random((A, ng)) < gt_ignore_p})
        evals.append(E)
    return evals


def test_symbol_declared_bound_and_exported():
    lib_mod, CE = _mod("_lib"), _mod("coco_eval")
    L = lib_mod.lib()
    assert "mrcnn_coco_accumulate" in lib_mod.EXPORTED_SYMBOLS and hasattr(L, "mrcnn_coco_accumulate")
    assert len(L.mrcnn_coco_accumulate.argtypes) == 17
    header = _header()
    assert "MRCNN_ERR_INVALID = %d," % INVALID in header and "MRCNN_ERR_SHAPE = %d," % SHAPE in header
    assert "mrcnn_coco_accumulate(" in header and "MRCNN_COCO_ACC_CHUNK %d" % CE.ACC_CHUNK in header
    for fn in (CE.score, CE.score_batch, CE._finish, _mod("evaluate").evaluate_coco_scored):
        assert inspect.signature(fn).parameters["accumulate_on"].default is None
    assert list(inspect.signature(CE.accumulate_device).parameters)[:5] == list(inspect.signature(CE.accumulate).parameters)
    with pytest.raises(ValueError):
        CE.score(CE.COCOGroundTruth({"images": [], "categories": [], "annotations": []}), [], accumulate_on="gpu")


def _tables():
    """Two categories (3 + 2 entries), A = 2, T = 2, M = 2, R = 3."""
    return {"scores": np.array([.9, .8, .7, .6, .5]), "ranks": np.array([0, 1, 2, 0, 1], np.int32), "matched": np.ones((2, 2, 5), np.uint8),
            "ignore": np.zeros((2, 2, 5), np.uint8), "offs": np.array([0, 3, 5], np.int64), "npig": np.array([[2, 1], [1, 0]], np.int64),
            "max_dets": np.array([1, 10], np.int32), "thr": np.array([0.0, 0.5, 1.0]), "precision": np.zeros((2, 3, 2, 2, 2)),
            "recall": np.zeros((2, 2, 2, 2))}


def _call(t, n_dt=5, K=2, A=2, T=2, M=2, R=3, memspace=0, **replace):
    t = dict(t, **replace)
    p = lambda a: None if a is None else a.ctypes.data
    L = _mod("_lib").lib()
    st = L.mrcnn_coco_accumulate(p(t["scores"]), p(t["ranks"]), p(t["matched"]), p(t["ignore"]), n_dt, p(t["offs"]), K, p(t["npig"]), A, T,
                                 p(t["max_dets"]), M, p(t["thr"]), R, memspace, p(t["precision"]), p(t["recall"]))
    return st, L.mrcnn_last_error().decode()


def test_argument_errors_come_before_the_device():
    t = _tables()
    for name in ("scores", "ranks", "matched", "ignore", "offs", "npig", "max_dets", "thr", "precision", "recall"):
        st, msg = _call(t, **{name: None})
        assert st == INVALID and "null" in msg, (name, st, msg)
    assert _call(t, n_dt=-1)[0] == INVALID and _call(t, K=-1)[0] == INVALID and _call(t, memspace=2)[0] == INVALID
    # the offsets
    st, msg = _call(t, offs=np.array([0, 4, 3], np.int64))
    assert st == INVALID and "category 1" in msg
    st, msg = _call(t, offs=np.array([1, 3, 5], np.int64))
    assert st == INVALID and "cat_offsets[0]" in msg
    st, msg = _call(t, offs=np.array([0, 3, 4], np.int64))
    assert st == INVALID and "end at 4" in msg
    st, msg = _call(t, npig=np.array([[2, 1], [-1, 0]], np.int64))
    assert st == INVALID and "category 1, area range 0" in msg
    # the sizes
    for name in ("A", "T", "M", "R"):
        for bad in (0, -2):
            st, msg = _call(t, **{name: bad})
            assert st == SHAPE and "at least 1" in msg, (name, bad, st, msg)
    st, msg = _call(t, thr=np.array([0.0, 0.6, 0.5]))
    assert st == SHAPE and "rec_thrs decrease at 1" in msg
    assert _call(t, thr=np.array([0.0, np.nan, 0.5]))[0] == SHAPE
    # the outputs of a refused call are untouched
    assert not t["precision"].any() and not t["recall"].any()


@pytest.mark.parametrize("max_dets", [(1, 10, 100), (1, 2, 5)])
def test_pack_evals_is_accumulates_own_concatenation(max_dets):
    CE = _mod("coco_eval")
    A, T = 4, 10
    evals = random_evals(np.random.default_rng(44), A=A, T=T)
    P = CE.pack_evals(evals, max_dets)
    cap = max(max_dets)
    assert P["scores"].dtype == np.float64 and P["ranks"].dtype == np.int32 and P["matched"].dtype == np.uint8 and P["ignore"].dtype == np.uint8
    assert P["cat_offsets"].dtype == np.int64 and P["npig"].dtype == np.int64 and P["npig"].shape == (len(evals), A)
    assert all(P[k].flags["C_CONTIGUOUS"] for k in P)
    assert P["cat_offsets"][0] == 0 and P["cat_offsets"][-1] == P["scores"].size == P["matched"].shape[2] and P["matched"].shape[:2] == (A, T)
    cut = 0
    for k, E in enumerate(evals):
        s0, s1 = int(P["cat_offsets"][k]), int(P["cat_offsets"][k + 1])
        if not E:
            assert s0 == s1 and not P["npig"][k].any()
            continue
        cut += sum(len(e["scores"]) > cap for e in E)
        np.testing.assert_array_equal(P["scores"][s0:s1], np.concatenate([e["scores"][:cap] for e in E]))
        np.testing.assert_array_equal(P["ranks"][s0:s1], np.concatenate([np.arange(min(cap, len(e["scores"]))) for e in E]))
        for a in range(A):
            np.testing.assert_array_equal(P["matched"][a, :, s0:s1], np.concatenate([e["matched"][a][:, :cap] for e in E], axis=1))
            np.testing.assert_array_equal(P["ignore"][a, :, s0:s1], np.concatenate([e["ignore"][a][:, :cap] for e in E], axis=1))
            assert P["npig"][k, a] == np.count_nonzero(np.concatenate([e["gt_ignore"][a] for e in E]) == 0)
    assert (cut > 0) == (cap == 5)                               # the cut records exist where the cut applies
    # nothing at all
    Z = CE.pack_evals([[], []], max_dets)
    assert Z["scores"].size == 0 and Z["matched"].shape == (A, T, 0) and Z["cat_offsets"].tolist() == [0, 0, 0] and Z["npig"].shape == (2, A)
    with pytest.raises(ValueError):
        CE.pack_evals(evals, max_dets, n_thrs=T + 1)
