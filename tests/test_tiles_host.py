"""Tiled prediction, the parts that need no GPU: the four entries' presence, the C example, the window planner, every argument error of
the three other entries, the host merge (mrcnn_merge_tiles_host, the DEFINITION of the device merge) against a brute-force
restatement on dense planes written here, and the round trip of the source-frame rows.  Every comparison is exact."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import tiles_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mrcnn_tile_plan", "mrcnn_maskrcnn_predict_tiles", "mrcnn_merge_tiles", "mrcnn_merge_tiles_host")
INVALID, HIP, SHAPE = 1, 3, 4


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


# ---- ABI and C host --------------------------------------------------------------------------------
def test_the_entries_are_declared_listed_and_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "maskrcnn_hip.h")).read()
    lib_mod = _lib()
    for sym in NEW_SYMBOLS:
        assert re.search(r"MRCNN_API\s+int\s+%s\s*\(" % sym, hdr), sym
        assert sym in lib_mod.EXPORTED_SYMBOLS, sym
    raw = C.CDLL(lib_mod.SO_PATH)
    for sym in NEW_SYMBOLS:
        assert hasattr(raw, sym), f"{sym} is not exported by libmaskrcnn_hip.so"
    L = lib_mod.lib()
    assert len(L.mrcnn_merge_tiles.argtypes) == 24 and len(L.mrcnn_merge_tiles_host.argtypes) == 23
    assert C.sizeof(lib_mod.Tile) == 20
    assert re.search(r"#define\s+MRCNN_TILES_MAX_CANDIDATES\s+%d\b" % lib_mod.TILES_MAX_CANDIDATES, hdr) and lib_mod.TILES_MAX_CANDIDATES >= 64 * 100
    for name in ("tile_plan", "merge_tiles", "merge_tiles_host"):
        assert callable(getattr(_det(), name))
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    assert callable(models.MaskRCNN.predict_tiles) and callable(models.MaskRCNN.predict_tiled)


def test_the_c_example_compiles(tmp_path):
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "mask-rcnn-coreml_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, os.path.join(ROOT, "examples", "maskrcnn_predict_tiled.c"), "-L", libdir,
           "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(tmp_path / "tiled")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


# ---- the planner -----------------------------------------------------------------------------------
def _check_axis(starts, L, T, O):
    assert all(0 <= s and s + min(T, L) <= L for s in starts)                     # inside
    if L <= T:
        assert starts == [0]
        return
    n = -(-(L - T) // (T - O)) + 1
    assert len(starts) == n                                                          # the formula
    covered = np.zeros(L, bool)
    for s in starts:
        covered[s:s + T] = True
    assert covered.all()                                                             # the union covers the axis
    assert all(a < b for a, b in zip(starts, starts[1:]))
    assert all(a + T - b >= O for a, b in zip(starts, starts[1:]))                   # neighbours share at least O


@pytest.mark.parametrize("h,w,th,tw,oy,ox", [(100, 90, 128, 128, 32, 32), (128, 128, 128, 128, 32, 0), (129, 128, 128, 128, 32, 32),
                                              (300, 257, 128, 64, 0, 0), (140, 200, 128, 16, 127, 15), (200, 333, 128, 128, 32, 32),
                                              (1, 1, 1, 1, 0, 0), (32767, 5, 4096, 8, 64, 3)])
def test_tile_plan(pkg, h, w, th, tw, oy, ox):
    tiles = _det().tile_plan(h, w, (th, tw), (oy, ox), image=7)
    assert tiles.dtype == np.int32 and tiles.shape[1] == 5 and (tiles[:, 0] == 7).all()
    np.testing.assert_array_equal(tiles, np.where(np.arange(5) == 0, 7, TC.plan(h, w, th, tw, oy, ox)))
    ys, xs = sorted(set(tiles[:, 1].tolist())), sorted(set(tiles[:, 2].tolist()))
    _check_axis(ys, h, th, oy)
    _check_axis(xs, w, tw, ox)
    assert (tiles[:, 3] == min(th, h)).all() and (tiles[:, 4] == min(tw, w)).all()  # exactly T long when L >= T
    np.testing.assert_array_equal(tiles[:, 1:3], [[y, x] for y in ys for x in xs])   # row-major, y outer
    if (h, w) == (200, 333):
        assert ys == [0, 72] and xs == [0, 96, 192, 205]                             # the last ones shifted inward


def test_tile_plan_protocol_and_errors(pkg):
    lib = _lib()
    L = lib.lib()
    n = C.c_int(-1)
    assert L.mrcnn_tile_plan(200, 333, 128, 128, 32, 32, 0, None, 0, C.byref(n)) == 0 and n.value == 8          # the size query
    buf = (lib.Tile * 8)()
    assert L.mrcnn_tile_plan(200, 333, 128, 128, 32, 32, 0, buf, 7, C.byref(n)) == SHAPE and n.value == 8
    assert L.mrcnn_tile_plan(200, 333, 128, 128, 32, 32, 0, buf, 8, C.byref(n)) == 0
    assert (buf[7].y0, buf[7].x0, buf[7].height, buf[7].width) == (72, 205, 128, 128)
    for bad in ((200, 333, 128, 128, 128, 32), (200, 333, 128, 128, -1, 0), (200, 333, 128, 128, 0, 128), (0, 333, 128, 128, 0, 0),
                (200, 32768, 128, 128, 0, 0), (200, 333, 0, 128, 0, 0), (200, 333, 128, 32768, 0, 0)):
        assert L.mrcnn_tile_plan(*bad, 0, None, 0, C.byref(n)) == SHAPE, bad
    assert L.mrcnn_tile_plan(200, 333, 128, 128, 32, 32, 0, None, 0, None) == INVALID


# ---- argument errors, answered without a device ----------------------------------------------------------------
def _merge_call(lib, host, sc, **over):
    T, rows = sc["det"].shape[:2]
    B = len(sc["sizes"])
    a = dict(det=sc["det"].ctypes.data, masks=sc["masks"].ctypes.data, tiles=sc["tiles"], n_tiles=T, rows=rows, S=TC.S,
             hs=np.array([s[0] for s in sc["sizes"]], np.int32), ws=np.array([s[1] for s in sc["sizes"]], np.int32), B=B, H=TC.MODEL, W=TC.MODEL,
             metric=lib.MATCH_IOS, thr=0.5, max_out=4)
    a.update(over)
    slots = max(1, a["B"] * max(1, a["max_out"]))
    src, source, nk = np.zeros((slots, 6), np.float32), np.zeros(slots, np.int32), np.zeros(max(1, a["B"]), np.int32)
    counts, offs = np.zeros(4096, np.uint32), np.zeros(slots + 1, np.int64)
    out = dict(src=src.ctypes.data, source=source.ctypes.data, nk=nk.ctypes.data, counts=counts.ctypes.data, cap=4096, offs=offs.ctypes.data)
    out.update({k: v for k, v in over.items() if k in out})
    tiles = np.ascontiguousarray(a["tiles"], np.int32) if a["tiles"] is not None else None
    tp = tiles.ctypes.data_as(C.POINTER(lib.Tile)) if tiles is not None else None
    head = (a["det"], a["masks"], tp, a["n_tiles"], a["rows"], a["S"], a["hs"].ctypes.data if a["hs"] is not None else None,
            a["ws"].ctypes.data if a["ws"] is not None else None, a["B"], a["H"], a["W"], C.c_float(0.5), a["metric"], a["thr"], a["max_out"])
    tail = (out["src"], out["source"], out["nk"], out["counts"], out["cap"], out["offs"], None, None)
    L = lib.lib()
    st = L.mrcnn_merge_tiles_host(*head, *tail) if host else L.mrcnn_merge_tiles(*head, lib.HOST, *tail)
    return st, L.mrcnn_last_error().decode()


@pytest.mark.parametrize("host", [True, False])
def test_merge_argument_errors_need_no_device(pkg, host):
    lib = _lib()
    sc = TC.scenes()[0]
    t = sc["tiles"]

    def moved(i, col, v):
        m = t.copy(); m[i, col] = v
        return m
    for over, code, word in [(dict(det=None), INVALID, "null"), (dict(masks=None), INVALID, "null"), (dict(tiles=None), INVALID, "null"),
                             (dict(hs=None), INVALID, "null"), (dict(src=None), INVALID, "null"), (dict(source=None), INVALID, "null"),
                             (dict(nk=None), INVALID, "null"), (dict(offs=None), INVALID, "null"), (dict(counts=None), INVALID, "counts"),
                             (dict(metric=2), INVALID, "metric"), (dict(thr=0.0), INVALID, "match_threshold"), (dict(thr=float("nan")), INVALID, "match_threshold"),
                             (dict(n_tiles=0), SHAPE, "n_tiles"), (dict(max_out=0), SHAPE, "max_out"), (dict(rows=0), SHAPE, "rows"),
                             (dict(tiles=moved(1, 0, 1)), SHAPE, "tile 1"), (dict(tiles=moved(1, 0, -1)), SHAPE, "tile 1"),
                             (dict(tiles=moved(1, 2, 97)), SHAPE, "tile 1"), (dict(tiles=moved(0, 1, -1)), SHAPE, "tile 0"),
                             (dict(tiles=moved(1, 3, 0)), SHAPE, "tile 1"), (dict(tiles=moved(0, 4, 0)), SHAPE, "tile 0"),
                             (dict(hs=np.array([40000], np.int32)), SHAPE, "image 0")]:
        st, msg = _merge_call(lib, host, sc, **over)
        assert st == code and word in msg, (over, st, msg)
    # the per-image candidate limit: 83 windows of one image x 100 rows
    many = np.tile(t[:1], (83, 1))
    st, msg = _merge_call(lib, host, sc, tiles=many, n_tiles=83, rows=100, det=np.zeros((83, 100, 6), np.float32).ctypes.data,
                          masks=np.zeros((83, 100, TC.S, TC.S), np.float32).ctypes.data)
    assert st == SHAPE and "8300 candidates" in msg and str(lib.TILES_MAX_CANDIDATES) in msg


def test_predict_tiles_argument_errors_need_no_device(pkg):
    lib = _lib()
    L = lib.lib()
    img = np.zeros((128, 224, 3), np.uint8)
    table = (lib.Image * 1)()
    table[0].rgb, table[0].height, table[0].width = img.ctypes.data, 128, 224
    tiles = np.array([[0, 0, 0, 128, 128], [0, 0, 96, 128, 128]], np.int32)
    tp = lambda t: np.ascontiguousarray(t, np.int32).ctypes.data_as(C.POINTER(lib.Tile))
    det, mask = np.zeros((2, 16, 6), np.float32), np.zeros((2, 16, 28, 28), np.float32)
    fake = C.c_void_p(16)                                        # never dereferenced: every check below comes before the handle is used
    err = lambda: L.mrcnn_last_error().decode()
    assert L.mrcnn_maskrcnn_predict_tiles(None, table, 1, tp(tiles), 2, lib.HOST, det.ctypes.data, mask.ctypes.data) == INVALID
    assert L.mrcnn_maskrcnn_predict_tiles(fake, None, 1, tp(tiles), 2, lib.HOST, det.ctypes.data, mask.ctypes.data) == INVALID
    assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, None, 2, lib.HOST, det.ctypes.data, mask.ctypes.data) == INVALID
    assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, tp(tiles), 2, lib.HOST, None, mask.ctypes.data) == INVALID
    assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, tp(tiles), 2, lib.HOST, det.ctypes.data, None) == INVALID
    assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, tp(tiles), 0, lib.HOST, det.ctypes.data, mask.ctypes.data) == SHAPE and "n_tiles" in err()
    for bad, word in [((1, 0, 1), "tile 1"), ((1, 0, -1), "tile 1"), ((1, 2, 97), "tile 1"), ((0, 1, 1), "tile 0"), ((1, 3, 0), "tile 1"), ((0, 4, -5), "tile 0")]:
        t = tiles.copy(); t[bad[0], bad[1]] = bad[2]
        assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, tp(t), 2, lib.HOST, det.ctypes.data, mask.ctypes.data) == SHAPE and word in err(), (bad, err())
    table[0].rgb = None
    assert L.mrcnn_maskrcnn_predict_tiles(fake, table, 1, tp(tiles), 2, lib.HOST, det.ctypes.data, mask.ctypes.data) == INVALID and "image 0" in err()


def test_the_device_merge_has_no_cpu_fallback(pkg):
    import torch
    st, msg = _merge_call(_lib(), False, TC.scenes()[0])
    assert st == (0 if torch.cuda.is_available() else HIP), (st, msg)


# ---- the host merge against a brute-force restatement on dense planes ------------------------------------------------
def brute_force(orc, ev, sc, metric, match_threshold, max_out):
    """The header's rule, as directly as it can be said: the oracle's numpy paste of every row on its tile, embedded in a dense plane
    of the full image; dense intersections; the greedy walk."""
    tiles, det, masks, rows = sc["tiles"], sc["det"], sc["masks"], sc["rows"]
    cands = []
    for t, (img, y0, x0, th, tw) in enumerate(tiles.tolist()):
        h, w = sc["sizes"][img]
        src = ev.unletterbox_boxes(det[t], th, tw, TC.MODEL, TC.MODEL).astype(np.float32)                   # the tile-frame rows
        planes = orc.paste_masks(src, masks[t], th, tw, 0.5)
        for i in range(rows):
            r = src[i]
            by1, bx1 = int(np.around(np.float64(r[0]) * (th - 1))), int(np.around(np.float64(r[1]) * (tw - 1)))
            by2, bx2 = int(np.around(np.float64(r[2]) * (th - 1) + 1.0)), int(np.around(np.float64(r[3]) * (tw - 1) + 1.0))
            eligible = bool(r[5] > 0) and by2 > by1 and bx2 > bx1
            full = np.zeros((h, w), np.uint8)
            row = np.zeros(6, np.float32)
            if eligible:
                full[y0:y0 + th, x0:x0 + tw] = planes[i]
                hy, wx = max(h - 1, 1), max(w - 1, 1)
                row[:] = [np.float32((by1 + y0) / hy), np.float32((bx1 + x0) / wx), np.float32((by2 + y0 - 1) / hy), np.float32((bx2 + x0 - 1) / wx), r[4], r[5]]
            cands.append(dict(k=t * rows + i, t=t, img=img, ok=eligible, plane=full, row=row, box=(by1 + y0, bx1 + x0, by2 + y0, bx2 + x0)))
    B = len(sc["sizes"])
    det_src, source, n_kept = np.zeros((B, max_out, 6), np.float32), np.full((B, max_out), -1, np.int32), np.zeros(B, np.int32)
    kept_planes = [[np.zeros(sc["sizes"][b], np.uint8) for _ in range(max_out)] for b in range(B)]
    for b in range(B):
        order = sorted((c for c in cands if c["img"] == b and c["ok"]), key=lambda c: (-float(c["row"][5]), c["k"]))
        kept = []
        for c in order:
            def m(q):
                inter = int(np.logical_and(q["plane"], c["plane"]).sum())
                aq, ac = int(q["plane"].sum()), int(c["plane"].sum())
                den = aq + ac - inter if metric == "iou" else min(aq, ac)
                return 0.0 if den == 0 else inter / den
            if not any(q["row"][4] == c["row"][4] and q["t"] != c["t"] and m(q) >= match_threshold for q in kept):
                kept.append(c)
        n_kept[b] = len(kept)
        for j, c in enumerate(kept[:max_out]):
            det_src[b, j], source[b, j], kept_planes[b][j] = c["row"], c["k"], c["plane"]
    return det_src, source, n_kept, kept_planes, cands


@pytest.fixture(scope="module")
def all_scenes(pkg):
    return TC.scenes()


def _configs(sc):
    cfgs = [(sc["metric"], sc["match_threshold"], sc["max_out"]), ("iou", 0.5, sc["max_out"]), ("ios", 0.5, sc["max_out"]), ("iou", 0.75, 2)]
    return list(dict.fromkeys(cfgs + [(m, t, sc["max_out"]) for (m, t) in sc["expect"]]))


def test_merge_host_equals_the_brute_force(pkg, orc, all_scenes):
    D, CR = _det(), importlib.import_module("mask-rcnn-coreml_amd.coco_results")
    ev = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
    names = [sc["name"] for sc in all_scenes]
    for need in ("duplicate_two_scores", "duplicate_two_classes", "same_tile_overlap", "cut_copy", "exactly_the_threshold", "duplicate_score_tie", "chain",
                 "max_out_below_kept", "tiles_larger_than_the_model", "tiles_smaller_than_the_model", "inward_shifted_edge_tiles", "two_images"):
        assert need in names
    dropped_somewhere = truncated = zero_area_kept = False
    for sc in all_scenes:
        for metric, thr, max_out in _configs(sc):
            want_src, want_source, want_n, want_planes, cands = brute_force(orc, ev, sc, metric, thr, max_out)
            src, source, n_kept, rles, areas, bboxes = D.merge_tiles_host(sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5,
                                                                           metric, thr, max_out)
            tag = (sc["name"], metric, thr, max_out)
            np.testing.assert_array_equal(source, want_source, err_msg=str(tag))
            np.testing.assert_array_equal(n_kept, want_n, err_msg=str(tag))
            np.testing.assert_array_equal(src.view(np.uint32), want_src.view(np.uint32), err_msg=str(tag))
            for b in range(len(sc["sizes"])):
                for j in range(max_out):
                    plane = want_planes[b][j]
                    np.testing.assert_array_equal(rles[b][j]["counts"], CR.rle_encode(plane)["counts"], err_msg=str(tag + (b, j)))
                    assert rles[b][j]["size"] == list(sc["sizes"][b])
                    assert int(areas[b, j]) == int(plane.sum())
                    ys, xs = np.nonzero(plane)
                    box = [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)] if ys.size else [0, 0, 0, 0]
                    assert bboxes[b, j].tolist() == box, tag
                    if source[b, j] >= 0 and ys.size == 0:
                        zero_area_kept = True
                    if source[b, j] >= 0:
                        # denorm_boxes of the source-frame row gives the full-frame pixel box back
                        h, w = sc["sizes"][b]
                        r = src[b, j].astype(np.float64)
                        got = (int(np.around(r[0] * (h - 1))), int(np.around(r[1] * (w - 1))), int(np.around(r[2] * (h - 1) + 1.0)), int(np.around(r[3] * (w - 1) + 1.0)))
                        assert got == cands[int(source[b, j])]["box"], tag
            if (metric, thr) in sc["expect"]:
                for b, keep in enumerate(sc["expect"][(metric, thr)]):
                    assert source[b][source[b] >= 0].tolist() == keep[:max_out] and n_kept[b] == len(keep), tag
            eligible = sum(c["ok"] for c in cands)
            dropped_somewhere |= int(n_kept.sum()) < eligible
            truncated |= bool((n_kept > max_out).any())
    assert dropped_somewhere and truncated and zero_area_kept


def test_merge_host_capacity_protocol(pkg, all_scenes):
    lib = _lib()
    sc = next(s for s in all_scenes if s["name"] == "cut_copy")
    slots = 4
    offs = np.zeros(slots + 1, np.int64)
    st, msg = _merge_call(lib, True, sc, counts=None, cap=0, offs=offs.ctypes.data)
    need = int(offs[slots])
    assert st == SHAPE and need > slots and f"capacity >= {need}" in msg                        # the size query: everything but counts is written
    counts = np.full(need + 1, 0xAAAAAAAA, np.uint32)
    st, msg = _merge_call(lib, True, sc, counts=counts.ctypes.data, cap=need - 1, offs=offs.ctypes.data)
    assert st == SHAPE and (counts == 0xAAAAAAAA).all()
    st, msg = _merge_call(lib, True, sc, counts=counts.ctypes.data, cap=need, offs=offs.ctypes.data)
    assert st == 0 and counts[need] == 0xAAAAAAAA and int(counts[:need].astype(np.int64).sum()) == slots * 128 * 224
    assert counts[int(offs[3])] == 128 * 224 and offs[4] == offs[3] + 1                         # a padding slot: the single run [h*w]


def test_source_rows_round_trip(pkg):
    """For full-frame pixel boxes with sides up to 32767, denorm_boxes of the row the merge writes — the four double quotients rounded
    to float once — returns the box: the error of the rounding is at most 32767 * 2^-24 of a pixel."""
    rng = np.random.default_rng(11)
    for _ in range(20000):
        h, w = (int(v) for v in rng.integers(1, 32768, 2))
        if rng.random() < 0.2:
            h, w = 32767, 32767
        y1, x1 = int(rng.integers(0, h)), int(rng.integers(0, w))
        y2, x2 = int(rng.integers(y1 + 1, h + 1)), int(rng.integers(x1 + 1, w + 1))
        hy, wx = max(h - 1, 1), max(w - 1, 1)
        r = np.array([y1 / hy, x1 / wx, (y2 - 1) / hy, (x2 - 1) / wx], np.float64).astype(np.float32).astype(np.float64)
        got = (int(np.around(r[0] * (h - 1))), int(np.around(r[1] * (w - 1))), int(np.around(r[2] * (h - 1) + 1.0)), int(np.around(r[3] * (w - 1) + 1.0)))
        assert got == (y1, x1, y2, x2), (h, w, y1, x1, y2, x2)
