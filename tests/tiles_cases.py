"""Scenes for the tile merge (mrcnn_merge_tiles / mrcnn_merge_tiles_host), shared by tests/test_tiles_host.py and
tests/test_gpu_tiles.py.  A scene is a dict: sizes [(h, w)] of the full images, tiles (T, 5) int32, det (T, rows, 6) in each tile's
LETTERBOXED frame at the model size MODEL x MODEL, masks (T, rows, S, S), and the merge's parameters metric / match_threshold /
max_out.  `expect` (optional) maps (metric, match_threshold) to the candidates that must be kept per image, in order.

The rows are built backwards from the pixel box wanted in the tile: for a tile of the model's size the letterbox is the identity and
the box comes out exactly; for other sizes it comes out within a pixel, which is all those scenes need."""
import ctypes as C
import importlib

import numpy as np

MODEL = 128
S = 28


def _geometry(h, w):
    lib = importlib.import_module("mask-rcnn-coreml_amd._lib")
    nh, nw, py, px = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    lib.check(lib.lib().mrcnn_letterbox_geometry(h, w, MODEL, MODEL, C.byref(nh), C.byref(nw), C.byref(py), C.byref(px)))
    return nh.value, nw.value, py.value, px.value


def row_for(tile_h, tile_w, box, cls, score):
    """The letterboxed-frame row whose pixel box in a tile_h x tile_w tile is (about) box = (y1, x1, y2, x2), far edges exclusive."""
    nh, nw, py, px = _geometry(tile_h, tile_w)
    sy, sx = tile_h / nh, tile_w / nw
    y1, x1, y2, x2 = box
    r = [(y1 / sy + py) / (MODEL - 1), (x1 / sx + px) / (MODEL - 1), (y2 / sy + py - 1.0) / (MODEL - 1), (x2 / sx + px - 1.0) / (MODEL - 1)]
    return np.array([min(max(v, 0.0), 1.0) for v in r] + [cls, score], np.float32)


def mask_of(kind, seed=0):
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    if kind == "full":
        return np.full((S, S), 0.9, np.float32)
    if kind == "none":
        return np.full((S, S), 0.1, np.float32)                 # below the threshold everywhere: a plane of area 0
    if kind == "disk":
        r2 = ((yy - 13.5) / 12.0) ** 2 + ((xx - 13.5) / 12.0) ** 2
        return np.where(r2 <= 1.0, 0.9, 0.1).astype(np.float32)
    rng = np.random.default_rng(seed)                           # "blob": smooth noise around the threshold, holes and islands
    g = rng.random((7, 7)).astype(np.float32)
    return np.kron(g, np.ones((4, 4), np.float32)) * 0.6 + 0.2


def scene(name, sizes, tiles, rows, entries, metric="ios", match_threshold=0.5, max_out=None, expect=None):
    """entries: (tile, row, box in the tile, class, score, mask kind[, seed])"""
    tiles = np.asarray(tiles, np.int32).reshape(-1, 5)
    T = tiles.shape[0]
    det = np.zeros((T, rows, 6), np.float32)
    masks = np.zeros((T, rows, S, S), np.float32)
    for e in entries:
        t, i, box, cls, score, kind = e[:6]
        det[t, i] = row_for(int(tiles[t, 3]), int(tiles[t, 4]), box, cls, score)
        masks[t, i] = mask_of(kind, e[6] if len(e) > 6 else 0)
    return dict(name=name, sizes=sizes, tiles=tiles, rows=rows, det=det, masks=masks, metric=metric, match_threshold=match_threshold,
                max_out=rows if max_out is None else max_out, expect=expect or {})


def _objects(name, sizes, tiles, rows, objects, seed, **kw):
    """Every object (image, full-frame box, class, score, mask kind) becomes a row in each tile that sees a part of it: whole where the
    window holds it, cut at the window's edge elsewhere — the duplicates tiling produces.  Scores differ a little from tile to tile."""
    rng = np.random.default_rng(seed)
    tiles = np.asarray(tiles, np.int32).reshape(-1, 5)
    fill = [0] * tiles.shape[0]
    entries = []
    for j, (img, (y1, x1, y2, x2), cls, score, kind) in enumerate(objects):
        for t, (ti, ty, tx, th, tw) in enumerate(tiles):
            if ti != img or fill[t] >= rows:
                continue
            cy1, cx1, cy2, cx2 = max(y1, ty), max(x1, tx), min(y2, ty + th), min(x2, tx + tw)
            if cy2 - cy1 < 2 or cx2 - cx1 < 2:
                continue
            entries.append((t, fill[t], (cy1 - ty, cx1 - tx, cy2 - ty, cx2 - tx), cls, score - 0.001 * float(rng.integers(0, 3)), kind, j))
            fill[t] += 1
    return scene(name, sizes, tiles, rows, entries, **kw)


def plan(h, w, th, tw, oy, ox, image=0):
    """The planner's rule, restated (tests/test_tiles_host.py checks mrcnn_tile_plan against it)."""
    def axis(L, T, O):
        if L <= T:
            return [0]
        s = T - O
        n = -(-(L - T) // s) + 1
        return [min(k * s, L - T) for k in range(n)]
    return np.array([[image, y, x, min(th, h), min(tw, w)] for y in axis(h, th, oy) for x in axis(w, tw, ox)], np.int32)


def scenes():
    two = [[0, 0, 0, 128, 128], [0, 0, 96, 128, 128]]            # two windows of a 128 x 224 image, 32 columns shared
    wide = [(128, 224)]
    k = lambda t, i, rows=4: t * rows + i
    out = []
    # the same object seen by both windows (the paste only sees pixel - box origin: equal masks give equal planes)
    dup = lambda c0, c1, s0, s1: [(0, 0, (30, 100, 70, 124), c0, s0, "disk"), (1, 1, (30, 4, 70, 28), c1, s1, "disk")]
    out.append(scene("duplicate_two_scores", wide, two, 4, dup(3, 3, 0.8, 0.9),
                     expect={("iou", 0.5): [[k(1, 1)]], ("ios", 0.5): [[k(1, 1)]]}))
    out.append(scene("duplicate_two_classes", wide, two, 4, dup(3, 4, 0.8, 0.9),
                     expect={("iou", 0.5): [[k(1, 1), k(0, 0)]], ("ios", 0.5): [[k(1, 1), k(0, 0)]]}))
    out.append(scene("duplicate_score_tie", wide, two, 4, dup(3, 3, 0.75, 0.75),
                     expect={("iou", 0.5): [[k(0, 0)]], ("ios", 0.5): [[k(0, 0)]]}))
    out.append(scene("same_tile_overlap", wide, two, 4, [(0, 0, (30, 40, 70, 80), 5, 0.9, "full"), (0, 1, (32, 42, 72, 82), 5, 0.8, "full")],
                     expect={("iou", 0.5): [[k(0, 0), k(0, 1)]], ("ios", 0.5): [[k(0, 0), k(0, 1)]]}))
    # the whole object in window 0 (60 columns), its cut copy in window 1 (24 columns): IoU 24/60 = 0.4, IoS 1
    out.append(scene("cut_copy", wide, two, 4, [(0, 0, (20, 60, 90, 120), 2, 0.95, "full"), (1, 0, (20, 0, 90, 24), 2, 0.9, "full"),
                                                  (0, 1, (100, 10, 120, 30), 2, 0.5, "none")],
                     expect={("iou", 0.5): [[k(0, 0), k(1, 0), k(0, 1)]], ("ios", 0.5): [[k(0, 0), k(0, 1)]]}))
    # 40 columns against 20 of them: IoU = 20h / 40h = 0.5 exactly — at the threshold the candidate is dropped
    out.append(scene("exactly_the_threshold", wide, two, 4, [(0, 0, (30, 88, 70, 128), 2, 0.9, "full"), (1, 0, (30, 0, 70, 20), 2, 0.8, "full")],
                     metric="iou", expect={("iou", 0.5): [[k(0, 0)]], ("iou", 0.75): [[k(0, 0), k(1, 0)]]}))
    # A drops B; B would have dropped C but suppresses nothing; A and C do not meet
    three = [[0, 0, 0, 128, 128], [0, 0, 48, 128, 128], [0, 0, 96, 128, 128]]
    out.append(scene("chain", wide, three, 4, [(0, 0, (30, 60, 70, 100), 2, 0.9, "full"), (1, 0, (30, 32, 70, 72), 2, 0.8, "full"),
                                               (2, 0, (30, 4, 70, 44), 2, 0.7, "full")],
                     expect={("ios", 0.5): [[k(0, 0), k(2, 0)]], ("iou", 0.5): [[k(0, 0), k(1, 0), k(2, 0)]]}))
    # more kept than max_out
    out.append(scene("max_out_below_kept", wide, two, 4, [(0, i, (10 + 25 * i, 10, 30 + 25 * i, 50), 1, 0.9 - 0.1 * i, "disk") for i in range(4)] +
                     [(1, i, (10 + 25 * i, 80, 30 + 25 * i, 120), 1, 0.85 - 0.1 * i, "blob", i) for i in range(3)], max_out=3))
    # windows larger and smaller than the model's input, windows shifted inward at the edges, two images in one call
    objs = [(0, (20, 30, 150, 140), 1, 0.9, "disk"), (0, (100, 150, 290, 255), 2, 0.8, "blob"), (0, (5, 180, 60, 250), 1, 0.7, "blob"),
            (0, (200, 10, 280, 120), 3, 0.6, "disk"), (0, (120, 100, 180, 190), 2, 0.85, "full")]
    big = np.array([[0, 0, 0, 300, 200], [0, 0, 60, 300, 200]], np.int32)
    out.append(_objects("tiles_larger_than_the_model", [(300, 260)], big, 6, objs, 1))
    small = plan(200, 333, 96, 160, 24, 40)
    objs2 = [(0, (10, 20, 90, 150), 1, 0.9, "disk"), (0, (60, 100, 180, 260), 2, 0.8, "blob"), (0, (100, 250, 199, 332), 1, 0.7, "disk"),
             (0, (0, 0, 50, 60), 3, 0.65, "full"), (0, (150, 5, 198, 110), 2, 0.6, "blob")]
    out.append(_objects("tiles_smaller_than_the_model", [(200, 333)], small, 5, objs2, 2))
    edge = plan(200, 333, 128, 128, 32, 32)                      # its last row and column of windows are shifted inward
    assert edge[-1, 1] == 200 - 128 and edge[-1, 2] == 333 - 128
    out.append(_objects("inward_shifted_edge_tiles", [(200, 333)], edge, 5, objs2, 3, metric="iou"))
    both = np.concatenate([plan(200, 333, 128, 128, 32, 32, 1), np.array(two, np.int32), plan(200, 333, 128, 128, 32, 32, 1)[:2]])
    objs3 = [(1,) + o[1:] for o in objs2] + [(0, (30, 90, 100, 130), 4, 0.9, "disk"), (0, (10, 10, 60, 60), 4, 0.5, "blob")]
    out.append(_objects("two_images", [(128, 224), (200, 333)], both, 6, objs3, 4, max_out=4))
    return out
