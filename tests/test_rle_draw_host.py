"""Drawing run-length masks, the parts that need no GPU: the six entries (mrcnn_rle_decode, mrcnn_instance_map_rle,
mrcnn_render_detections_rle and their _host definitions) are declared, listed, exported and bound; a plain C host calls the three
definitions and the new example compiles; the definitions equal coco_results.rle_decode and the numpy restatement of
tests/test_render_host.py (`restate` on `pixel_boxes`, fed the decoded planes) on the outputs of the host merge and the host union
for every scene of tests/unite_cases.py; the inputs have teeth; and every argument error is answered without a device."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import tiles_cases as TC
import unite_cases as UC
from test_render_host import PALETTE, pixel_boxes, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW_SYMBOLS = ("mrcnn_rle_decode", "mrcnn_rle_decode_host", "mrcnn_instance_map_rle", "mrcnn_instance_map_rle_host",
               "mrcnn_render_detections_rle", "mrcnn_render_detections_rle_host")
INVALID, HIP, SHAPE = 1, 3, 4


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_listed_exported_and_bound(pkg):
    hdr = open(os.path.join(INC, "maskrcnn_hip.h")).read()
    lib_mod = _lib()
    raw = C.CDLL(lib_mod.SO_PATH)
    for sym in NEW_SYMBOLS:
        assert re.search(r"MRCNN_API\s+int\s+%s\s*\(" % sym, hdr), sym
        assert sym in lib_mod.EXPORTED_SYMBOLS, sym
        assert hasattr(raw, sym), f"{sym} is not exported by libmaskrcnn_hip.so"
    L = lib_mod.lib()
    assert len(L.mrcnn_rle_decode.argtypes) == 9 and len(L.mrcnn_rle_decode_host.argtypes) == 8
    assert len(L.mrcnn_instance_map_rle.argtypes) == 12 and len(L.mrcnn_instance_map_rle_host.argtypes) == 11
    assert len(L.mrcnn_render_detections_rle.argtypes) == 12 and len(L.mrcnn_render_detections_rle_host.argtypes) == 11
    for name in ("rle_decode_planes", "instance_map_rle", "render_detections_rle"):
        assert callable(getattr(_det(), name)) and callable(getattr(_det(), name + "_host"))
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    for name in ("render_tiled", "render_tiled_jpegs", "instance_pngs_tiled"):
        assert callable(getattr(models.MaskRCNN, name))
    assert "cannot reproduce it" not in hdr and "mrcnn_render_detections_rle (below)" in hdr
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "entries for RLE input" not in " ".join(readme.split())


def test_a_c_host_calls_the_three_definitions(tmp_path):
    src = tmp_path / "draw_rle.c"
    src.write_text(
        '#include "maskrcnn_hip.h"\n'
        "int run(const uint8_t* rgb, const float* det_src, const uint32_t* counts, const int64_t* run_offsets, uint8_t* planes, int16_t* map,\n"
        "        uint32_t* visible, uint8_t* out)\n"
        "{\n"
        "    mrcnn_image image;\n"
        "    const int32_t heights[1] = {480}, widths[1] = {640};\n"
        "    const int64_t offsets[1] = {0};\n"
        "    int st;\n"
        "    image.rgb = rgb; image.height = 480; image.width = 640;\n"
        "    st = mrcnn_rle_decode_host(counts, run_offsets, 1, 100, heights, widths, planes, offsets);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_instance_map_rle_host(det_src, counts, run_offsets, 1, 100, heights, widths, 0.0f, map, offsets, visible);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_instance_map_rle_host(det_src, counts, run_offsets, 1, 100, heights, widths, 0.0f, map, offsets, NULL);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_render_detections_rle_host(&image, det_src, counts, run_offsets, 1, 100, 0.7f, 128, 3, out, offsets);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_rle_decode(counts, run_offsets, 1, 100, heights, widths, MRCNN_HOST, planes, offsets);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_instance_map_rle(det_src, counts, run_offsets, 1, 100, heights, widths, 0.0f, MRCNN_HOST, map, offsets, visible);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    return mrcnn_render_detections_rle(&image, det_src, counts, run_offsets, 1, 100, 0.7f, 128, 3, MRCNN_HOST, out, offsets);\n"
        "}\n")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_the_example_host_builds(pkg, tmp_path):
    libdir = os.path.dirname(_lib().SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_render_tiled.c")
    text = open(src).read()
    assert "mrcnn_unite_tiles" in text and "mrcnn_render_detections_rle" in text and "mrcnn_jpeg_encode_batch" in text
    exe = str(tmp_path / "maskrcnn_render_tiled")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "usage" in r.stderr


# ---- decode ------------------------------------------------------------------------------------------------------------------
def _rle(h, w, counts):
    return {"size": [h, w], "counts": np.asarray(counts, np.uint32)}


def decode_cases():
    """(name, rle): every RLE sums to its plane."""
    CR = _cr()
    rng = np.random.default_rng(20261019)
    out = [("full", _rle(5, 7, [0, 35])), ("empty", _rle(5, 7, [35])),
           ("checkerboard", _rle(6, 9, [1] * 54)), ("checkerboard_from_one", _rle(6, 9, [0] + [1] * 54)),
           ("runs_cross_columns", _rle(128, 224, [7680, 12800, 8192])),
           ("zero_run_first", _rle(4, 5, [0, 3, 17])), ("zero_run_middle", _rle(4, 5, [2, 3, 0, 4, 11])), ("zero_run_last", _rle(4, 5, [2, 18, 0])),
           ("zero_runs_everywhere", _rle(4, 5, [0, 0, 0, 3, 0, 0, 5, 0, 12, 0, 0])),
           ("one_row", _rle(1, 9, [2, 3, 1, 3])), ("one_column", _rle(9, 1, [0, 4, 5])), ("one_pixel_set", _rle(1, 1, [0, 1])), ("one_pixel_clear", _rle(1, 1, [1]))]
    for k, (h, w, p) in enumerate([(37, 53, 0.5), (64, 200, 0.1), (33, 257, 0.9), (2, 3, 0.5)]):
        out.append((f"random_{k}", CR.rle_encode(rng.random((h, w)) < p)))
    return out


def test_decode_equals_rle_decode(pkg):
    D, CR = _det(), _cr()
    for name, rle in decode_cases():
        got = D.rle_decode_planes_host([[rle]])
        assert len(got) == 1 and got[0].dtype == np.uint8 and got[0].shape == (1, *rle["size"]), name
        np.testing.assert_array_equal(got[0][0], CR.rle_decode(rle), err_msg=name)
    # a ragged set: two slots per image, three images, and the (counts, run_offsets) form with run_offsets[0] > 0 (a subset)
    cases = dict(decode_cases())
    rles = [[cases["random_0"], CR.rle_encode(np.zeros((37, 53)))], [cases["random_1"], CR.rle_encode(np.ones((64, 200)))], [cases["one_pixel_set"], cases["one_pixel_clear"]]]
    got = D.rle_decode_planes_host(rles)
    for b in range(3):
        for i in range(2):
            np.testing.assert_array_equal(got[b][i], CR.rle_decode(rles[b][i]))
    counts = np.concatenate([[9, 9, 9]] + [r["counts"] for row in rles for r in row]).astype(np.uint32)
    offs = np.concatenate(([3], 3 + np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
    got = D.rle_decode_planes_host((counts, offs), sizes=[(37, 53), (64, 200), (1, 1)])
    for b in range(3):
        for i in range(2):
            np.testing.assert_array_equal(got[b][i], CR.rle_decode(rles[b][i]))
    sub = D.rle_decode_planes_host((counts, offs[3:5]), sizes=[(64, 200)])      # "run_offsets + first with a smaller slots"
    np.testing.assert_array_equal(sub[0][0], CR.rle_decode(rles[1][1]))


# ---- map and render against the restatement -----------------------------------------------------------------------------------
def _source(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def tiled_results(pkg):
    """(tag, det_src (B, slots, 6), rles, sizes, planes per image) from the host merge and the host union of every unite_cases scene."""
    D, CR = _det(), _cr()
    out = []
    for sc in UC.scenes():
        args = (sc["det"], sc["masks"], sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5)
        for tag, res in (("merge", D.merge_tiles_host(*args, "ios", 0.5, sc["max_out"])), ("unite", D.unite_tiles_host(*args, "iou", 0.5, sc["max_out"]))):
            det_src, rles = res[0], res[3]
            planes = [np.stack([CR.rle_decode(r) for r in row]) for row in rles]
            out.append((f"{sc['name']}/{tag}", det_src, rles, [tuple(s) for s in sc["sizes"]], planes))
            if sc["name"] == "chain" and tag == "unite":
                # a user's own boxes on the same masks: every box shrunk to its middle half, so each mask has set pixels outside its box
                # (the merge's and the union's own boxes always hold their masks)
                own = det_src.copy()
                cy, cx = (own[..., 0] + own[..., 2]) / 2, (own[..., 1] + own[..., 3]) / 2
                hy, hx = (own[..., 2] - own[..., 0]) / 4, (own[..., 3] - own[..., 1]) / 4
                own[..., 0], own[..., 1], own[..., 2], own[..., 3] = cy - hy, cx - hx, cy + hy, cx + hx
                out.append(("chain/unite/own_boxes", own, rles, [tuple(s) for s in sc["sizes"]], planes))
    return out


def _min_scores(det_src):
    """Two cuts: below every score, and one that removes a drawn row where the scene has two different scores."""
    s = np.unique(det_src[..., 5][det_src[..., 5] > 0])
    return [0.0, float(s[len(s) // 2]) if len(s) else 0.5]


def test_the_map_equals_the_restatement(tiled_results):
    D = _det()
    for tag, det_src, rles, sizes, planes in tiled_results:
        for min_score in _min_scores(det_src):
            maps, visible = D.instance_map_rle_host(det_src, rles, min_score=min_score)
            assert visible.dtype == np.uint32 and visible.shape == det_src.shape[:2]
            for b, (h, w) in enumerate(sizes):
                want = restate(pixel_boxes(det_src[b], h, w), det_src[b, :, 5], planes[b], min_score)
                assert maps[b].dtype == np.int16
                np.testing.assert_array_equal(maps[b], want[0], err_msg=f"{tag} image {b} min_score {min_score}")
                np.testing.assert_array_equal(visible[b], want[1], err_msg=f"{tag} image {b} min_score {min_score}")


@pytest.mark.parametrize("alpha", [0, 128, 256])
@pytest.mark.parametrize("stroke", [0, 1, 3])
def test_the_render_equals_the_restatement(tiled_results, alpha, stroke):
    D = _det()
    for n, (tag, det_src, rles, sizes, planes) in enumerate(tiled_results):
        images = [_source(h, w, 100 * n + b) for b, (h, w) in enumerate(sizes)]
        for min_score in _min_scores(det_src):
            got = D.render_detections_rle_host(images, det_src, rles, min_score=min_score, alpha=alpha, stroke=stroke)
            for b, (h, w) in enumerate(sizes):
                want = restate(pixel_boxes(det_src[b], h, w), det_src[b, :, 5], planes[b], min_score, stroke, alpha, images[b])[3]
                assert got[b].dtype == np.uint8 and got[b].shape == (h, w, 3)
                np.testing.assert_array_equal(got[b], want, err_msg=f"{tag} image {b} min_score {min_score}")


def test_the_box_only_decides_whether_a_row_is_drawn(pkg):
    """A user's own box need not be tight: set pixels outside it count, an empty box or a score of 0 draws nothing."""
    D, CR = _det(), _cr()
    plane = np.zeros((10, 12), np.uint8); plane[2:9, 1:11] = 1
    rles = [[CR.rle_encode(plane)] * 3]
    det = np.zeros((1, 3, 6), np.float32)
    det[0, 0] = [0.5, 0.5, 0.5, 0.5, 1, 0.0]                                    # score 0
    det[0, 1] = [0.6, 0.6, 0.2, 0.9, 1, 0.9]                                    # inverted box
    det[0, 2] = [4 / 9, 5 / 11, 5 / 9, 6 / 11, 1, 0.8]                          # a 2x2 box inside the mask
    maps, visible = D.instance_map_rle_host(det, rles)
    np.testing.assert_array_equal(visible, [[0, 0, 70]])
    np.testing.assert_array_equal(maps[0], np.where(plane != 0, 2, -1))
    want = restate(pixel_boxes(det[0], 10, 12), det[0, :, 5], np.stack([plane] * 3), 0.0)
    np.testing.assert_array_equal(maps[0], want[0])


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
def test_the_inputs_have_teeth(tiled_results):
    """Each property the comparisons above rest on holds for at least one of their cases."""
    contested = outside = padding = cut = ring_over_fill = False
    for tag, det_src, rles, sizes, planes in tiled_results:
        for b, (h, w) in enumerate(sizes):
            boxes, scores = pixel_boxes(det_src[b], h, w), det_src[b, :, 5]
            padding |= bool((scores == 0).any() and (planes[b][scores == 0].sum() == 0))
            for min_score in _min_scores(det_src):
                inst, visible, ring, _ = restate(boxes, scores, planes[b], min_score, stroke=3)
                drawn = [i for i in range(len(scores)) if scores[i] > np.float32(min_score) and scores[i] > 0 and boxes[i][2] > boxes[i][0] and boxes[i][3] > boxes[i][1]]
                cut |= any(0 < scores[i] <= np.float32(min_score) and planes[b][i].any() for i in range(len(scores)))
                cover = sum((planes[b][i] != 0).astype(np.int32) for i in drawn) if drawn else np.zeros((h, w), np.int32)
                last = max(drawn) if drawn else -1
                contested |= bool(((cover > 1) & (inst != last) & (inst >= 0)).any())
                for i in drawn:
                    y1, x1, y2, x2 = boxes[i]
                    inside = np.zeros((h, w), bool); inside[max(y1, 0):y2, max(x1, 0):x2] = True
                    outside |= bool(((planes[b][i] != 0) & ~inside).any())
                ring_over_fill |= bool(((ring >= 0) & (inst >= 0)).any())
    assert contested, "no contested pixel whose owner is not the last row"
    assert outside, "no drawn row with set pixels outside its box"
    assert padding, "no padding slot"
    assert cut, "no row cut off by min_score"
    assert ring_over_fill, "no ring pixel over a fill pixel"


# ---- errors, answered without a device --------------------------------------------------------------------------------------------
def _call(entry, host, **over):
    """One call of `entry` ('decode', 'map', 'render') on a 4x5 image with two RLEs; keyword arguments replace single arguments."""
    lib = _lib()
    L = lib.lib()
    a = dict(counts=np.array([2, 3, 15, 0, 20], np.uint32), offs=np.array([0, 3, 5], np.int64), B=1, slots=2, hs=np.array([4], np.int32), ws=np.array([5], np.int32),
             det=np.array([[0, 0, 1, 1, 1, 0.9], [0, 0, 1, 1, 1, 0.8]], np.float32), min_score=0.0, alpha=128, stroke=3, out_offs=np.array([0], np.int64),
             img=np.full((4, 5, 3), 7, np.uint8), out=np.full(256, 0x5a, np.uint8), visible=np.full(2, 77, np.uint32))
    a.update(over)
    p = lambda v: None if v is None else v.ctypes.data
    table = (lib.Image * max(1, a["B"]))()                  # the render takes its sizes from the image table; every entry shows the one buffer
    for b in range(a["B"]):
        table[b].rgb, table[b].height, table[b].width = p(a["img"]), int(a["hs"][b]), int(a["ws"][b])
    space = () if host else (lib.HOST,)
    suffix = "_host" if host else ""
    if entry == "decode":
        st = getattr(L, "mrcnn_rle_decode" + suffix)(p(a["counts"]), p(a["offs"]), a["B"], a["slots"], p(a["hs"]), p(a["ws"]), *space, p(a["out"]), p(a["out_offs"]))
    elif entry == "map":
        st = getattr(L, "mrcnn_instance_map_rle" + suffix)(p(a["det"]), p(a["counts"]), p(a["offs"]), a["B"], a["slots"], p(a["hs"]), p(a["ws"]), C.c_float(a["min_score"]),
                                                           *space, p(a["out"]), p(a["out_offs"]), p(a["visible"]))
    else:
        st = getattr(L, "mrcnn_render_detections_rle" + suffix)(table, p(a["det"]), p(a["counts"]), p(a["offs"]),
                                                                a["B"], a["slots"], C.c_float(a["min_score"]), a["alpha"], a["stroke"], *space, p(a["out"]), p(a["out_offs"]))
    return st, L.mrcnn_last_error().decode(), a


@pytest.mark.parametrize("host", [True, False])
@pytest.mark.parametrize("entry", ["decode", "map", "render"])
def test_argument_errors_need_no_device(pkg, entry, host):
    big = lambda v: np.array([v], np.int32)
    st, msg, _ = _call(entry, host, out=None)
    assert st == INVALID, msg
    st, msg, _ = _call(entry, host, offs=None)
    assert st == INVALID, msg
    st, msg, _ = _call(entry, host, out_offs=None)
    assert st == INVALID, msg
    st, msg, _ = _call(entry, host, out_offs=np.array([8], np.int64))
    assert st == INVALID and "multiple of 16" in msg, msg
    st, msg, _ = _call(entry, host, out_offs=np.array([-16], np.int64))
    assert st == INVALID, msg
    if entry != "decode":
        st, msg, _ = _call(entry, host, det=None)
        assert st == INVALID, msg
        st, msg, _ = _call(entry, host, slots=32768)
        assert st == SHAPE and "32767" in msg, msg
    if entry == "render":
        st, msg, _ = _call(entry, host, img=None)
        assert st == INVALID and "rgb" in msg, msg
        for bad in (dict(alpha=-1), dict(alpha=257), dict(stroke=-1), dict(stroke=65535)):
            st, msg, _ = _call(entry, host, **bad)
            assert st == SHAPE, (bad, msg)
    for bad in (dict(hs=big(0)), dict(ws=big(0)), dict(hs=big(32768)), dict(ws=big(32768))):
        st, msg, _ = _call(entry, host, **bad)
        assert st == SHAPE and "1..32767" in msg, (bad, msg)
    # two images whose ranges overlap in the output
    st, msg, _ = _call(entry, host, B=2, slots=1, hs=np.array([4, 4], np.int32), ws=np.array([5, 5], np.int32), out_offs=np.array([0, 16], np.int64))
    assert st == INVALID and "overlap" in msg, msg


@pytest.mark.parametrize("entry", ["decode", "map", "render"])
def test_a_bad_rle_is_named_and_nothing_is_written(pkg, entry):
    for counts, k in ((np.array([2, 3, 15, 0, 21], np.uint32), 1), (np.array([2, 3, 14, 0, 20], np.uint32), 0), (np.array([2, 3, 15, 0, 19], np.uint32), 1)):
        st, msg, a = _call(entry, True, counts=counts)
        assert st == SHAPE and f"RLE {k} " in msg and "20" in msg, msg
        assert (a["out"] == 0x5a).all() and (a["visible"] == 77).all()
    st, msg, a = _call(entry, True, offs=np.array([0, 3, 2], np.int64))
    assert st == SHAPE and "decrease" in msg and (a["out"] == 0x5a).all(), msg
    st, msg, a = _call(entry, True)
    assert st == 0 and not (a["out"] == 0x5a).all(), msg


def test_the_device_entries_have_no_cpu_fallback(pkg):
    import torch
    for entry in ("decode", "map", "render"):
        st, msg, _ = _call(entry, False)
        assert st == (0 if torch.cuda.is_available() else HIP), (entry, st, msg)
