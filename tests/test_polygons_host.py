"""Run-length masks to polygon rings, the parts that need no GPU: mrcnn_rle_to_polygons and its _host definition are declared, listed,
exported and bound; the definition equals the naive restatement of tests/polygons_cases.py in every array, on every mask of 3x3 and 2x2,
300 random masks, lines, full and empty planes, checkerboards, a hole with an island and two RLEs that are not in normal form; the rings
have the properties the header states; mrcnn_rle_from_polygons, the rasteriser this library already trusts, gives the masks back; the
capacity protocol, the argument errors and a bad RLE are answered without a device; a plain C host calls the definition, the example
builds, and coco_results writes COCO polygons."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import polygons_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW_SYMBOLS = ("mrcnn_rle_to_polygons", "mrcnn_rle_to_polygons_host")
INVALID, HIP, SHAPE = PC.INVALID, PC.HIP, PC.SHAPE


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _cr():
    return importlib.import_module("mask-rcnn-coreml_amd.coco_results")


@pytest.fixture(scope="module")
def traced(pkg):
    """every case once: (names, rles, planes, the host definition's arrays, the restatement per RLE)"""
    names = [n for n, _ in PC.cases()]
    rles = [r for _, r in PC.cases()]
    planes = [_cr().rle_decode(r) for r in rles]
    return names, rles, planes, PC.trace_host(rles), [PC.restate(p) for p in planes]


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
    assert len(L.mrcnn_rle_to_polygons.argtypes) == 15 and len(L.mrcnn_rle_to_polygons_host.argtypes) == 14
    m = re.search(r"#define\s+MRCNN_POLYGON_LDS_CORNERS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == lib_mod.POLYGON_LDS_CORNERS
    assert callable(_det().rle_to_polygons) and callable(_det().rle_to_polygons_host)
    for word in ("Douglas-Peucker", "smoothing", "sub-pixel", "visits it once"):
        assert word in hdr, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "**Polygons out.**" in readme and "api_polygons.hip" in readme and "Douglas" in readme
    assert "mrcnn_rle_to_polygons" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "polygons_ab.py" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_a_c_host_calls_the_definition(tmp_path):
    src = tmp_path / "polygons.c"
    src.write_text(
        '#include "maskrcnn_hip.h"\n'
        "int run(const uint32_t* counts, const int64_t* run_offsets, int64_t* rle_rings, int64_t* ring_offsets, int64_t* ring_areas, int32_t* xy)\n"
        "{\n"
        "    const int32_t heights[1] = {480}, widths[1] = {640};\n"
        "    int64_t rings = 0, vertices = 0;\n"
        "    int st = mrcnn_rle_to_polygons_host(counts, run_offsets, 1, 100, heights, widths, rle_rings, &rings, &vertices, NULL, NULL, 0, NULL, 0);\n"
        "    if (st != MRCNN_OK && st != MRCNN_ERR_SHAPE) return st;\n"
        "    st = mrcnn_rle_to_polygons_host(counts, run_offsets, 1, 100, heights, widths, rle_rings, &rings, &vertices, ring_offsets, ring_areas, rings, xy, vertices);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    return mrcnn_rle_to_polygons(counts, run_offsets, 1, 100, heights, widths, MRCNN_HOST, rle_rings, &rings, &vertices, ring_offsets, NULL,\n"
        "                                 MRCNN_POLYGON_LDS_CORNERS, xy, vertices);\n"
        "}\n")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_the_example_host_builds_and_traces_without_a_device(pkg, tmp_path):
    libdir = os.path.dirname(_lib().SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_polygons.c")
    text = open(src).read()
    assert "mrcnn_rle_to_polygons(" in text and "mrcnn_rle_to_polygons_host(" in text
    exe = str(tmp_path / "maskrcnn_polygons")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "usage" in r.stderr
    # a 4 x 5 plane with a hole, as a file: "h w n" and the runs; --host asks for the definition, which needs no device
    plane = np.ones((4, 5), np.uint8)
    plane[1:3, 1:3] = 0
    rle = _cr().rle_encode(plane)
    f = tmp_path / "set.txt"
    f.write_text("1 1\n4 5 %d\n%s\n" % (len(rle["counts"]), " ".join(str(int(c)) for c in rle["counts"])))
    r = subprocess.run([exe, "--host", str(f)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0].split()[:4] == ["2", "rings,", "8", "vertices"], lines
    assert "area 20: 0,0 5,0 5,4 0,4" in lines[1] and "area -4: 1,1 1,3 3,3 3,1" in lines[2], lines


# ---- the definition against the restatement -------------------------------------------------------------------------------------
def test_the_definition_equals_the_restatement_in_every_array(traced):
    names, _rles, _planes, got, want = traced
    assert len(names) >= 512 + 16 + 300 + 10
    for k, name in enumerate(names):                             # per mask first: a difference is named
        g_rings, g_areas = PC.rings_of(got, k)
        w_rings, w_areas = want[k]
        assert len(g_rings) == len(w_rings), name
        for g, w in zip(g_rings, w_rings):
            np.testing.assert_array_equal(g, w, err_msg=name)
        np.testing.assert_array_equal(g_areas, w_areas, err_msg=name)
    PC.assert_same(got, PC.flat_arrays(want), "the whole set")
    assert got["xy"].dtype == np.int32 and got["ring_areas"].dtype == np.int64


def test_the_cases_reach_holes_and_diagonal_contacts(traced):
    names, _rles, _planes, got, _want = traced
    holes = twice = 0
    for k, name in enumerate(names):
        if not name.startswith("random/"):
            continue
        rings, areas = PC.rings_of(got, k)
        holes += bool((areas < 0).any())
        twice += sum(len({(int(x), int(y)) for x, y in r}) < len(r) for r in rings)
    assert holes >= 30 and twice >= 30, (holes, twice)


def test_not_in_normal_form_equals_normal_form(traced):
    names, rles, planes, got, _want = traced

    def cut_at_column_ends(rle):
        """every run cut where a column ends, the pieces joined by runs of length zero: one vertical interval per run of ones"""
        h, out, pos = rle["size"][0], [], 0
        for j, c in enumerate(int(c) for c in rle["counts"]):
            pieces = []
            while c > 0:
                step = min(c, h - pos % h)
                pieces.append(step)
                pos, c = pos + step, c - step
            out.extend(sum(([p, 0] for p in pieces), [])[:-1] if pieces else [0])
        return {"size": rle["size"], "counts": np.array(out, np.uint32)}

    for name, other in (("zero_length_runs", _cr().rle_encode), ("crossing_column_ends", lambda p: cut_at_column_ends(_cr().rle_encode(p)))):
        k = names.index(name)
        normal = other(planes[k])
        np.testing.assert_array_equal(_cr().rle_decode(normal), planes[k])
        again = PC.trace_host([normal])
        assert planes[k].any() and len(rles[k]["counts"]) != len(normal["counts"])
        rings, areas = PC.rings_of(got, k)
        w_rings, w_areas = PC.rings_of(again, 0)
        assert len(rings) == len(w_rings) and all(np.array_equal(a, b) for a, b in zip(rings, w_rings)) and np.array_equal(areas, w_areas)


def test_the_properties_of_a_ring(traced):
    names, _rles, planes, got, _want = traced
    for k, name in enumerate(names):
        rings, areas = PC.rings_of(got, k)
        h, w = planes[k].shape
        assert int(areas.sum()) == int(planes[k].sum()), name                                     # the signed areas sum to the set pixels
        assert (areas != 0).all(), name
        starts = [(int(r[0, 0]), int(r[0, 1])) for r in rings]
        assert all(a < b for a, b in zip(starts, starts[1:])), name                                  # strictly increasing: no two rings share a start
        for r in rings:
            m = len(r)
            assert m >= 4 and m % 2 == 0, name
            assert (r[:, 0] >= 0).all() and (r[:, 0] <= w).all() and (r[:, 1] >= 0).all() and (r[:, 1] <= h).all(), name
            d = np.roll(r, -1, axis=0) - r                                                           # closed: the last piece returns to the start
            horizontal = (d[:, 1] == 0) & (d[:, 0] != 0)
            vertical = (d[:, 0] == 0) & (d[:, 1] != 0)
            assert (horizontal | vertical).all() and (horizontal[::2] == horizontal[0]).all() and (horizontal[1::2] != horizontal[0]).all(), name
            assert min((int(x), int(y)) for x, y in r) == (int(r[0, 0]), int(r[0, 1])), name
            assert sum((int(x), int(y)) == (int(r[0, 0]), int(r[0, 1])) for x, y in r) == 1, name    # the start is visited once
    assert got["n_rings"] == len(got["ring_areas"]) and got["n_vertices"] == len(got["xy"]) == got["ring_offsets"][-1]


# ---- round trip through the rasteriser ---------------------------------------------------------------------------------------------
def _rasterise(rings, h, w):
    """mrcnn_rle_from_polygons on the rings as one annotation -> counts"""
    L = _lib().lib()
    xy = np.concatenate(rings).astype(np.float64).reshape(-1)
    offs = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    n = C.c_int64(0)
    out = np.zeros(2 * h * w + 4, np.uint32)
    st = L.mrcnn_rle_from_polygons(xy.ctypes.data, offs.ctypes.data, len(rings), h, w, out.ctypes.data, out.size, C.byref(n))
    assert st == 0, L.mrcnn_last_error().decode()
    return out[:n.value].copy()


def test_every_ring_rasterised_alone_xors_to_the_mask(traced):
    names, _rles, planes, got, _want = traced
    CR = _cr()
    for k, name in enumerate(names):
        rings, _areas = PC.rings_of(got, k)
        h, w = planes[k].shape
        acc = np.zeros((h, w), np.uint8)
        for r in rings:
            acc ^= CR.rle_decode({"size": [h, w], "counts": _rasterise([r], h, w)})
        np.testing.assert_array_equal(acc, planes[k], err_msg=name)


def test_outlines_alone_give_the_rle_back_word_for_word(traced):
    names, _rles, planes, got, _want = traced
    CR = _cr()
    seen = 0
    for k, name in enumerate(names):
        rings, areas = PC.rings_of(got, k)
        if len(rings) == 0 or (areas < 0).any():
            continue
        seen += 1
        h, w = planes[k].shape
        np.testing.assert_array_equal(_rasterise(rings, h, w), CR.rle_encode(planes[k])["counts"], err_msg=name)
    assert seen >= 500


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def _one(name="hole_with_island"):
    rle = dict(PC.cases())[name]
    return PC.flatten([rle])


def test_the_size_query_and_buffers_that_are_too_small(pkg):
    counts, offs, hs, ws = _one()
    st, msg, q = PC.call_host(counts, offs, 1, 1, hs, ws, 0, 0, null=True)
    assert st == SHAPE and q["n_rings"] == 4 and q["n_vertices"] == 16 and list(q["rle_rings"]) == [0, 4], msg
    assert "ring_capacity >= 4" in msg and "vertex_capacity >= 16" in msg
    for rc, vc in ((3, 16), (4, 15), (0, 0)):
        st, msg, out = PC.call_host(counts, offs, 1, 1, hs, ws, rc, vc, fill=-9)
        assert st == SHAPE and "ring_capacity >= 4" in msg and "vertex_capacity >= 16" in msg, msg
        assert list(out["rle_rings"]) == [0, 4] and (out["n_rings"], out["n_vertices"]) == (4, 16)     # always written
        assert (out["ring_offsets"] == -9).all() and (out["ring_areas"] == -9).all() and (out["xy"] == -9).all()
    st, msg, out = PC.call_host(counts, offs, 1, 1, hs, ws, 6, 20, fill=-9)                            # larger than needed: the rest stays
    assert st == 0, msg
    assert list(out["ring_offsets"][:5]) == [0, 4, 8, 12, 16] and (out["ring_offsets"][5:] == -9).all() and (out["xy"][32:] == -9).all()
    assert list(out["ring_areas"][:4]) == [63, -35, 9, -1]
    # an empty set and a set of empty masks: no rings, the query succeeds
    empty = PC.flatten([dict(PC.cases())["empty"]] * 3)
    st, msg, q = PC.call_host(*empty[:2], 3, 1, *empty[2:], 0, 0, null=True)
    assert st == 0 and q["n_rings"] == 0 and q["n_vertices"] == 0 and list(q["rle_rings"]) == [0, 0, 0, 0], msg
    st, msg, q = PC.call_host(np.zeros(0, np.uint32), np.zeros(1, np.int64), 0, 5, np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0, null=True)
    assert st == 0 and q["n_rings"] == 0 and list(q["rle_rings"]) == [0], msg


@pytest.mark.parametrize("entry", ["mrcnn_rle_to_polygons_host", "mrcnn_rle_to_polygons"])
def test_argument_errors_need_no_device(pkg, entry):
    lib = _lib()
    L = lib.lib()
    counts, offs, hs, ws = _one()
    rle_rings, ro, ra, xy = np.zeros(2, np.int64), np.zeros(9, np.int64), np.zeros(8, np.int64), np.zeros(64, np.int32)
    nr, nv = C.c_int64(0), C.c_int64(0)

    def call(counts=counts, offs=offs, n_images=1, slots=1, hs=hs, ws=ws, memspace=lib.HOST, rle_rings=rle_rings, nr=C.byref(nr), nv=C.byref(nv),
             ro=ro, rc=8, xy=xy, vc=32):
        p = lambda a: None if a is None else a.ctypes.data
        mem = (memspace,) if entry == "mrcnn_rle_to_polygons" else ()
        st = getattr(L, entry)(p(counts), p(offs), n_images, slots, p(hs), p(ws), *mem, p(rle_rings), nr, nv, p(ro), ra.ctypes.data, rc, p(xy), vc)
        return st, L.mrcnn_last_error().decode()

    who = entry[len("mrcnn_"):]
    for kw in (dict(offs=None), dict(hs=None), dict(ws=None), dict(rle_rings=None), dict(nr=None), dict(nv=None), dict(ro=None), dict(xy=None),
               dict(n_images=-1), dict(slots=-1), dict(rc=-1), dict(vc=-1)):
        st, msg = call(**kw)
        assert st == INVALID and msg.startswith(who + ":"), (kw, msg)
    for side in (0, 32768):
        st, msg = call(hs=np.array([side], np.int32))
        assert st == SHAPE and "image 0" in msg and "1..32767" in msg, msg
    st, msg = call(offs=np.array([5, 2], np.int64))
    assert st == SHAPE and "run_offsets decrease at RLE 0" in msg, msg
    if entry == "mrcnn_rle_to_polygons":
        st, msg = call(memspace=7)
        assert st == INVALID and "memspace" in msg, msg


@pytest.mark.parametrize("entry", ["mrcnn_rle_to_polygons_host", "mrcnn_rle_to_polygons"])
def test_a_bad_rle_is_named_and_nothing_is_written(pkg, entry):
    lib = _lib()
    L = lib.lib()
    rles = [dict(PC.cases())[n] for n in ("full", "hole_with_island", "checkerboard")]
    counts, offs, hs, ws = PC.flatten(rles)
    for delta in (1, -1):
        bad = counts.copy()
        bad[offs[1] + 1] = np.uint32(int(bad[offs[1] + 1]) + delta)
        rle_rings, ro, ra, xy = np.full(4, -9, np.int64), np.full(65, -9, np.int64), np.full(64, -9, np.int64), np.full(512, -9, np.int32)
        nr, nv = C.c_int64(-9), C.c_int64(-9)
        mem = (lib.HOST,) if entry == "mrcnn_rle_to_polygons" else ()
        st = getattr(L, entry)(bad.ctypes.data, offs.ctypes.data, 3, 1, hs.ctypes.data, ws.ctypes.data, *mem, rle_rings.ctypes.data, C.byref(nr), C.byref(nv),
                               ro.ctypes.data, ra.ctypes.data, 64, xy.ctypes.data, 256)
        msg = L.mrcnn_last_error().decode()
        assert st == SHAPE and "RLE 1 (image 1, slot 0)" in msg and f"sums to {99 + delta} pixels" in msg and "9x11" in msg, msg
        assert (rle_rings == -9).all() and (ro == -9).all() and (ra == -9).all() and (xy == -9).all() and nr.value == -9 and nv.value == -9


def test_no_cpu_fallback_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib()
    with pytest.raises(lib.MrcnnError) as e:
        _det().rle_to_polygons([[dict(PC.cases())["full"]]])
    assert e.value.code == HIP


def test_the_python_entry_returns_rings_and_areas(pkg, traced):
    names, rles, _planes, got, _want = traced
    picked = [names.index(n) for n in ("hole_with_island", "checkerboard")]
    D = _det()
    rows = [[rles[picked[0]], {"size": [9, 11], "counts": np.array([99], np.uint32)}], [rles[picked[1]], rles[picked[1]]]]      # two images of two slots
    rings, areas = D.rle_to_polygons_host(rows)
    assert rings[0][1] == [] and len(areas[0][1]) == 0
    for (b, i), k in zip(((0, 0), (1, 0), (1, 1)), (picked[0], picked[1], picked[1])):
        w_rings, w_areas = PC.rings_of(got, k)
        assert len(rings[b][i]) == len(w_rings) and all(np.array_equal(a, c) for a, c in zip(rings[b][i], w_rings))
        np.testing.assert_array_equal(areas[b][i], w_areas)
    flat = D.rle_to_polygons_host(rows, flat=True)
    assert flat["n_rings"] == sum(len(r) for row in rings for r in row) and flat["xy"].shape == (flat["n_vertices"], 2)


# ---- COCO polygons ------------------------------------------------------------------------------------------------------------------
def test_coco_results_writes_outlines_as_polygons(pkg, traced):
    names, rles, _planes, _got, _want = traced
    CR, D = _cr(), _det()
    a, b = rles[names.index("hole_with_island")], rles[names.index("checkerboard")]
    big = {"size": [9, 11], "counts": np.array([0, 99], np.uint32)}
    rows = [[a, big], [b, b]]
    sizes = [(9, 11), (8, 9)]
    det = np.zeros((2, 2, 6), np.float32)
    det[:, :, :4] = [0, 0, 1, 1]
    det[:, :, 4] = 3
    det[:, :, 5] = [[0.9, 0.8], [0.7, 0.0]]
    before = CR.coco_results([7, 8], det, rows, sizes)
    assert CR.coco_results([7, 8], det, rows, sizes, segmentation="rle") == before and len(before) == 3
    assert all(set(r["segmentation"]) == {"size", "counts"} and isinstance(r["segmentation"]["counts"], str) for r in before)
    polys = D.rle_to_polygons_host(rows)
    got = CR.coco_results([7, 8], det, rows, sizes, segmentation="polygon", polygons=polys)
    assert [{k: v for k, v in r.items() if k != "segmentation"} for r in got] == [{k: v for k, v in r.items() if k != "segmentation"} for r in before]
    # the ring with a hole with an island: the two outlines stay, the two holes go
    assert got[0]["segmentation"] == [[1.0, 1.0, 10.0, 1.0, 10.0, 8.0, 1.0, 8.0], [4.0, 3.0, 7.0, 3.0, 7.0, 6.0, 4.0, 6.0]]
    assert got[1]["segmentation"] == [[0.0, 0.0, 11.0, 0.0, 11.0, 9.0, 0.0, 9.0]]
    assert len(got[2]["segmentation"]) == 36 and all(len(p) == 8 for p in got[2]["segmentation"])     # 36 single pixels
    assert all(isinstance(v, float) for r in got for p in r["segmentation"] for v in p)
    small = CR.coco_results([7, 8], det, rows, sizes, segmentation="polygon", min_area=10, polygons=polys)
    assert small[0]["segmentation"] == [[1.0, 1.0, 10.0, 1.0, 10.0, 8.0, 1.0, 8.0]] and small[2]["segmentation"] == []
    with pytest.raises(ValueError):
        CR.coco_results([7, 8], det, rows, sizes, segmentation="mask")
    import json
    json.dumps(got)
