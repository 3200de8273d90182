"""Uniting the cut parts of objects across tiles, the parts that need no GPU: the two entries' presence, the C example, the argument
errors, the capacity protocol, and the host definition (mrcnn_unite_tiles_host) against a brute-force restatement on dense boolean
planes written here, against the hand-derived numbers of tests/unite_cases.py and against mrcnn_merge_tiles_host where nothing can
link.  Every comparison is exact."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import tiles_cases as TC
import unite_cases as UC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mrcnn_unite_tiles", "mrcnn_unite_tiles_host")
INVALID, HIP, SHAPE = 1, 3, 4


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- ABI and C host --------------------------------------------------------------------------------
def test_the_entries_are_declared_listed_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "maskrcnn_hip.h")).read()
    lib_mod = _lib()
    raw = C.CDLL(lib_mod.SO_PATH)
    for sym in NEW_SYMBOLS:
        assert re.search(r"MRCNN_API\s+int\s+%s\s*\(" % sym, hdr), sym
        assert sym in lib_mod.EXPORTED_SYMBOLS, sym
        assert hasattr(raw, sym), f"{sym} is not exported by libmaskrcnn_hip.so"
    L = lib_mod.lib()
    assert len(L.mrcnn_unite_tiles.argtypes) == 26 and len(L.mrcnn_unite_tiles_host.argtypes) == 25
    assert len(L.mrcnn_merge_tiles.argtypes) == 24 and len(L.mrcnn_merge_tiles_host.argtypes) == 23          # unchanged
    for name in ("unite_tiles", "unite_tiles_host"):
        assert callable(getattr(_det(), name))
    assert "never united" not in hdr and "mrcnn_unite_tiles (below)" in hdr
    import inspect
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    p = inspect.signature(models.MaskRCNN.predict_tiled).parameters
    assert p["unite"].default is False and p["link_threshold"].default == 0.5


def test_the_c_example_compiles(pkg, tmp_path):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "mask-rcnn-coreml_amd")
    src = os.path.join(ROOT, "examples", "maskrcnn_predict_tiled.c")
    assert "mrcnn_unite_tiles" in open(src).read()
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
           "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "tiled")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


# ---- argument errors, answered without a device ----------------------------------------------------------------
def _unite_call(lib, host, sc, **over):
    T, rows = sc["det"].shape[:2]
    B = len(sc["sizes"])
    a = dict(det=sc["det"].ctypes.data, masks=sc["masks"].ctypes.data, tiles=sc["tiles"], n_tiles=T, rows=rows, S=TC.S,
             hs=np.array([s[0] for s in sc["sizes"]], np.int32), ws=np.array([s[1] for s in sc["sizes"]], np.int32), B=B, H=TC.MODEL, W=TC.MODEL,
             metric=lib.MATCH_IOU, thr=0.5, max_out=4)
    a.update(over)
    slots = max(1, a["B"] * max(1, a["max_out"]))
    src, source, nk = np.zeros((slots, 6), np.float32), np.zeros(slots, np.int32), np.zeros(max(1, a["B"]), np.int32)
    counts, offs = np.zeros(4096, np.uint32), np.zeros(slots + 1, np.int64)
    out = dict(src=src.ctypes.data, source=source.ctypes.data, nk=nk.ctypes.data, counts=counts.ctypes.data, cap=4096, offs=offs.ctypes.data,
               parts=None, group=None, areas=None, boxes=None)
    out.update({k: v for k, v in over.items() if k in out})
    tiles = np.ascontiguousarray(a["tiles"], np.int32) if a["tiles"] is not None else None
    tp = tiles.ctypes.data_as(C.POINTER(lib.Tile)) if tiles is not None else None
    head = (a["det"], a["masks"], tp, a["n_tiles"], a["rows"], a["S"], a["hs"].ctypes.data if a["hs"] is not None else None,
            a["ws"].ctypes.data if a["ws"] is not None else None, a["B"], a["H"], a["W"], C.c_float(0.5), a["metric"], a["thr"], a["max_out"])
    tail = (out["src"], out["source"], out["nk"], out["parts"], out["group"], out["counts"], out["cap"], out["offs"], out["areas"], out["boxes"])
    L = lib.lib()
    st = L.mrcnn_unite_tiles_host(*head, *tail) if host else L.mrcnn_unite_tiles(*head, lib.HOST, *tail)
    return st, L.mrcnn_last_error().decode()


@pytest.mark.parametrize("host", [True, False])
def test_unite_argument_errors_need_no_device(pkg, host):
    lib = _lib()
    sc = UC.scenes()[0]
    t = sc["tiles"]
    who = "unite_tiles_host" if host else "unite_tiles:"

    def moved(i, col, v):
        m = t.copy(); m[i, col] = v
        return m
    for over, code, word in [(dict(det=None), INVALID, "null"), (dict(masks=None), INVALID, "null"), (dict(tiles=None), INVALID, "null"),
                             (dict(hs=None), INVALID, "null"), (dict(ws=None), INVALID, "null"), (dict(src=None), INVALID, "null"),
                             (dict(source=None), INVALID, "null"), (dict(nk=None), INVALID, "null"), (dict(offs=None), INVALID, "null"),
                             (dict(counts=None), INVALID, "counts"), (dict(metric=2), INVALID, "metric"), (dict(thr=0.0), INVALID, "link_threshold"),
                             (dict(thr=-1.0), INVALID, "link_threshold"), (dict(thr=float("nan")), INVALID, "link_threshold"),
                             (dict(n_tiles=0), SHAPE, "n_tiles"), (dict(max_out=0), SHAPE, "max_out"), (dict(rows=0), SHAPE, "rows"),
                             (dict(B=0), SHAPE, "n_images"),
                             (dict(tiles=moved(1, 0, 1)), SHAPE, "tile 1"), (dict(tiles=moved(1, 0, -1)), SHAPE, "tile 1"),
                             (dict(tiles=moved(1, 2, 97)), SHAPE, "tile 1"), (dict(tiles=moved(0, 1, -1)), SHAPE, "tile 0"),
                             (dict(tiles=moved(1, 3, 0)), SHAPE, "tile 1"), (dict(tiles=moved(0, 4, 0)), SHAPE, "tile 0"),
                             (dict(hs=np.array([40000], np.int32)), SHAPE, "image 0")]:
        st, msg = _unite_call(lib, host, sc, **over)
        assert st == code and word in msg and msg.startswith(who), (over, st, msg)
    many = np.tile(t[:1], (83, 1))                               # the per-image candidate limit: 83 windows of one image x 100 rows
    st, msg = _unite_call(lib, host, sc, tiles=many, n_tiles=83, rows=100, det=np.zeros((83, 100, 6), np.float32).ctypes.data,
                          masks=np.zeros((83, 100, TC.S, TC.S), np.float32).ctypes.data)
    assert st == SHAPE and "8300 candidates" in msg and str(lib.TILES_MAX_CANDIDATES) in msg and msg.startswith(who)


def test_the_device_union_has_no_cpu_fallback(pkg):
    import torch
    st, msg = _unite_call(_lib(), False, UC.scenes()[0])
    assert st == (0 if torch.cuda.is_available() else HIP), (st, msg)


def test_unite_host_capacity_protocol(pkg):
    lib = _lib()
    sc = next(s for s in UC.scenes() if s["name"] == "cut_in_two")
    slots = 4
    offs, parts, group = np.zeros(slots + 1, np.int64), np.full(slots, -7, np.int32), np.full(8, -7, np.int32)
    areas = np.zeros(slots, np.uint32)
    st, msg = _unite_call(lib, True, sc, counts=None, cap=0, offs=offs.ctypes.data, parts=parts.ctypes.data, group=group.ctypes.data, areas=areas.ctypes.data)
    need = int(offs[slots])
    # the size query: everything but counts is written.  100 columns of 40 rows: 100 runs of ones, 101 of zeros; three padding slots
    assert st == SHAPE and need == 201 + 3 and f"capacity >= {need}" in msg
    assert parts.tolist() == [2, 0, 0, 0] and group.tolist() == [0, -1, -1, -1, 0, -1, -1, -1] and areas.tolist() == [4000, 0, 0, 0]
    counts = np.full(need + 1, 0xAAAAAAAA, np.uint32)
    st, msg = _unite_call(lib, True, sc, counts=counts.ctypes.data, cap=need - 1, offs=offs.ctypes.data)
    assert st == SHAPE and (counts == 0xAAAAAAAA).all()
    st, msg = _unite_call(lib, True, sc, counts=counts.ctypes.data, cap=need, offs=offs.ctypes.data)
    assert st == 0 and counts[need] == 0xAAAAAAAA and int(counts[:need].astype(np.int64).sum()) == slots * 128 * 224
    assert counts[int(offs[3])] == 128 * 224 and offs[4] == offs[3] + 1                           # a padding slot: the single run [h*w]


# ---- the definition against a brute-force restatement on dense planes ------------------------------------------------
def dense_candidates(orc, ev, sc):
    """The oracle's numpy paste of every row on its tile, embedded in a dense boolean plane of the full image."""
    tiles, det, masks, rows = sc["tiles"], sc["det"], sc["masks"], sc["rows"]
    cands = []
    for t, (img, y0, x0, th, tw) in enumerate(tiles.tolist()):
        h, w = sc["sizes"][img]
        src = ev.unletterbox_boxes(det[t], th, tw, TC.MODEL, TC.MODEL).astype(np.float32)
        planes = orc.paste_masks(src, masks[t], th, tw, 0.5)
        for i in range(rows):
            r = src[i]
            by1, bx1 = int(np.around(np.float64(r[0]) * (th - 1))), int(np.around(np.float64(r[1]) * (tw - 1)))
            by2, bx2 = int(np.around(np.float64(r[2]) * (th - 1) + 1.0)), int(np.around(np.float64(r[3]) * (tw - 1) + 1.0))
            ok = bool(r[5] > 0) and by2 > by1 and bx2 > bx1
            full = np.zeros((h, w), bool)
            if ok:
                full[y0:y0 + th, x0:x0 + tw] = planes[i] != 0
            cands.append(dict(k=t * rows + i, t=t, img=img, ok=ok, plane=full, cls=r[4], score=r[5], win=(y0, x0, y0 + th, x0 + tw),
                              box=(by1 + y0, bx1 + x0, by2 + y0, bx2 + x0)))
    return cands


def brute_force(cands, sc, metric, link_threshold, max_out):
    """The header's rule on dense planes: link, union-find, OR."""
    B = len(sc["sizes"])
    T, rows = sc["det"].shape[:2]
    det_src, source, n_kept = np.zeros((B, max_out, 6), np.float32), np.full((B, max_out), -1, np.int32), np.zeros(B, np.int32)
    n_parts, group = np.zeros((B, max_out), np.int32), np.full(T * rows, -1, np.int32)
    planes = [[np.zeros(sc["sizes"][b], bool) for _ in range(max_out)] for b in range(B)]
    links = 0
    for b in range(B):
        h, w = sc["sizes"][b]
        order = sorted((c for c in cands if c["img"] == b and c["ok"]), key=lambda c: (-float(c["score"]), c["k"]))
        parent = list(range(len(order)))

        def find(i):
            while parent[i] != i:
                i = parent[i]
            return i
        for i, c in enumerate(order):
            for j, q in enumerate(order[:i]):
                if q["cls"] != c["cls"] or q["t"] == c["t"]:
                    continue
                y0, x0, y1, x1 = max(q["win"][0], c["win"][0]), max(q["win"][1], c["win"][1]), min(q["win"][2], c["win"][2]), min(q["win"][3], c["win"][3])
                if y1 <= y0 or x1 <= x0:
                    continue
                inter = int((q["plane"] & c["plane"]).sum())
                aq, ac = int(q["plane"][y0:y1, x0:x1].sum()), int(c["plane"][y0:y1, x0:x1].sum())
                assert inter == int((q["plane"] & c["plane"])[y0:y1, x0:x1].sum())                         # inside R by construction
                den = aq + ac - inter if metric == "iou" else min(aq, ac)
                if (0.0 if den == 0 else inter / den) >= link_threshold:
                    links += 1
                    ri, rj = find(i), find(j)
                    parent[max(ri, rj)] = min(ri, rj)
        reps = [i for i in range(len(order)) if find(i) == i]                                              # ascending place = output order
        n_kept[b] = len(reps)
        for ci, rep in enumerate(reps):
            mem = [c for i, c in enumerate(order) if find(i) == rep]
            for c in mem:
                group[c["k"]] = ci
            if ci >= max_out:
                continue
            y1, x1 = min(c["box"][0] for c in mem), min(c["box"][1] for c in mem)
            y2, x2 = max(c["box"][2] for c in mem), max(c["box"][3] for c in mem)
            hy, wx = max(h - 1, 1), max(w - 1, 1)
            det_src[b, ci] = [np.float32(y1 / hy), np.float32(x1 / wx), np.float32((y2 - 1) / hy), np.float32((x2 - 1) / wx), mem[0]["cls"], mem[0]["score"]]
            source[b, ci], n_parts[b, ci] = mem[0]["k"], len(mem)
            for c in mem:
                planes[b][ci] |= c["plane"]
    return det_src, source, n_kept, planes, n_parts, group.reshape(T, rows), links


@pytest.fixture(scope="module")
def all_scenes(pkg):
    return UC.scenes()


@pytest.fixture(scope="module")
def dense(pkg, orc, all_scenes):
    ev = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
    return {sc["name"]: dense_candidates(orc, ev, sc) for sc in all_scenes}


def _run(sc, metric, thr, max_out):
    return _det().unite_tiles_host(sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, metric, thr, max_out)


def test_unite_host_equals_the_brute_force(all_scenes, dense):
    CR = _cr()
    linked = truncated = multi = chained = False
    for sc in all_scenes:
        for metric, thr, max_out in UC.configs(sc):
            w_src, w_source, w_n, w_planes, w_parts, w_group, links = brute_force(dense[sc["name"]], sc, metric, thr, max_out)
            src, source, n_kept, rles, areas, bboxes, n_parts, group = _run(sc, metric, thr, max_out)
            tag = (sc["name"], metric, thr, max_out)
            np.testing.assert_array_equal(source, w_source, err_msg=str(tag))
            np.testing.assert_array_equal(n_kept, w_n, err_msg=str(tag))
            np.testing.assert_array_equal(n_parts, w_parts, err_msg=str(tag))
            np.testing.assert_array_equal(group, w_group, err_msg=str(tag))
            np.testing.assert_array_equal(src.view(np.uint32), w_src.view(np.uint32), err_msg=str(tag))
            for b in range(len(sc["sizes"])):
                for j in range(max_out):
                    plane = w_planes[b][j].astype(np.uint8)
                    np.testing.assert_array_equal(rles[b][j]["counts"], CR.rle_encode(plane)["counts"], err_msg=str(tag + (b, j)))
                    assert rles[b][j]["size"] == list(sc["sizes"][b])
                    assert int(areas[b, j]) == int(plane.sum())
                    ys, xs = np.nonzero(plane)
                    box = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if ys.size else [0, 0, 0, 0]
                    assert bboxes[b, j].tolist() == box, tag
            linked |= links > 0
            truncated |= bool((n_kept > max_out).any())
            multi |= bool((n_parts > 1).any())
            chained |= bool((n_parts > 2).any())
    assert linked and truncated and multi and chained


def test_the_hand_derived_expectations(all_scenes):
    names = [sc["name"] for sc in all_scenes]
    for need in ("cut_in_two", "exactly_the_threshold", "neighbours", "full_height", "whole_and_cut", "classes_differ", "same_tile", "score_tie", "chain"):
        assert need in names
    checked = 0
    for sc in all_scenes:
        for (metric, thr), per_image in sc["unite"].items():
            src, source, n_kept, rles, areas, bboxes, n_parts, group = _run(sc, metric, thr, sc["max_out"])
            tag = (sc["name"], metric, thr)
            for b, comps in enumerate(per_image):
                assert n_kept[b] == len(comps), tag
                for j, c in enumerate(comps):
                    assert source[b, j] == c["members"][0] and n_parts[b, j] == len(c["members"]), tag
                    assert sorted(np.flatnonzero(group.reshape(-1) == j).tolist()) == sorted(c["members"]), tag
                    assert int(areas[b, j]) == c["area"] and tuple(bboxes[b, j].tolist()) == c["bbox"], tag
                    if "rle" in c:
                        assert rles[b][j]["counts"].tolist() == c["rle"], tag
                    checked += 1
                assert (source[b, len(comps):] == -1).all() and (n_parts[b, len(comps):] == 0).all()
    assert checked >= 14
    chain = next(sc for sc in all_scenes if sc["name"] == "chain")
    out = _run(chain, "iou", 0.5, 4)
    assert out[1][0, 0] == UC.k(1, 0) and out[0][0, 0, 5] == np.float32(0.9)
    h, w = chain["sizes"][0]
    np.testing.assert_array_equal(out[0][0, 0, :4], np.array([30 / (h - 1), 20 / (w - 1), 69 / (h - 1), 269 / (w - 1)], np.float64).astype(np.float32))


def test_why_uniting_is_needed(all_scenes):
    """The motivation, on cut_in_two: the merge either keeps ONE fragment (IoS = 1280 / 2560 = 0.5 drops the other) or reports both
    fragments as two instances (IoU = 1280 / 4000); the union reports one object of 4000 pixels."""
    D = _det()
    sc = next(s for s in all_scenes if s["name"] == "cut_in_two")
    args = (sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5)
    ios = D.merge_tiles_host(*args, "ios", 0.5, 4)
    assert ios[2][0] == 1 and ios[1][0].tolist() == [UC.k(0, 0), -1, -1, -1] and int(ios[4][0, 0]) == 2720
    iou = D.merge_tiles_host(*args, "iou", 0.5, 4)
    assert iou[2][0] == 2 and sorted(int(a) for a in iou[4][0, :2]) == [2560, 2720]
    one = D.unite_tiles_host(*args, "iou", 0.5, 4)
    assert one[2][0] == 1 and int(one[4][0, 0]) == 4000 and one[6][0].tolist() == [2, 0, 0, 0]


def test_nothing_links_above_one_and_the_output_is_the_merge(all_scenes):
    """No measure exceeds 1: with link_threshold 1.5 every component has one member, with match_threshold 1.5 the merge drops nothing,
    and the two outputs are the same bits."""
    D = _det()
    for sc in all_scenes:
        for metric in ("iou", "ios"):
            for max_out in (sc["max_out"], 2):
                args = (sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, metric, 1.5, max_out)
                m, u = D.merge_tiles_host(*args), D.unite_tiles_host(*args)
                tag = (sc["name"], metric, max_out)
                for a, b in zip(m[:3] + m[4:], u[:3] + u[4:6]):
                    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=str(tag))
                for mb, ub in zip(m[3], u[3]):
                    for x, y in zip(mb, ub):
                        np.testing.assert_array_equal(x["counts"], y["counts"], err_msg=str(tag))
                np.testing.assert_array_equal(u[6], (u[1] >= 0).astype(np.int32), err_msg=str(tag))


def test_every_output_plane_is_the_or_of_its_group(all_scenes):
    D, CR = _det(), _cr()
    for sc in all_scenes:
        T, rows = sc["det"].shape[:2]
        alone = D.unite_tiles_host(sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 1.5, T * rows)
        plane_of = {int(k): CR.rle_decode(alone[3][b][j]) for b in range(len(sc["sizes"])) for j, k in enumerate(alone[1][b]) if k >= 0}
        for metric, thr, max_out in UC.configs(sc):
            src, source, n_kept, rles, areas, bboxes, n_parts, group = _run(sc, metric, thr, max_out)
            assert set(np.flatnonzero(group.reshape(-1) >= 0).tolist()) == set(plane_of)
            for b in range(len(sc["sizes"])):
                of_image = [k for k in plane_of if sc["tiles"][k // rows, 0] == b]
                assert n_kept[b] == len({int(group.reshape(-1)[k]) for k in of_image})
                for j in range(max_out):
                    mem = [k for k in of_image if group.reshape(-1)[k] == j]
                    assert n_parts[b, j] == len(mem) and (source[b, j] in mem if mem else source[b, j] == -1)
                    want = np.zeros(sc["sizes"][b], np.uint8)
                    for k in mem:
                        want |= plane_of[k]
                    np.testing.assert_array_equal(CR.rle_decode(rles[b][j]), want, err_msg=str((sc["name"], metric, thr, max_out, b, j)))


def test_the_union_goes_to_the_coco_writers_unchanged(pkg, all_scenes):
    """masks_rle_source's layout: coco_results.coco_results takes det_src and the rles as they are."""
    CR = _cr()
    sc = next(s for s in all_scenes if s["name"] == "chain")
    src, source, n_kept, rles, areas, bboxes, n_parts, group = _run(sc, "iou", 0.5, 4)
    res = CR.coco_results([7], src, rles, sc["sizes"])
    assert len(res) == 1 and res[0]["image_id"] == 7 and res[0]["score"] == float(np.float32(0.9))
    back = CR.rle_decode({"size": res[0]["segmentation"]["size"], "counts": res[0]["segmentation"]["counts"]})
    assert int(back.sum()) == 10000 and [round(v) for v in res[0]["bbox"]] == [20, 30, 250, 40]
