"""examples/maskrcnn_polygons.c with --props: built the way tests/test_c_host_components.py builds it, run with --host (the definitions
need no device) on a small set, and compared with detection.rle_region_props_host; without the flag its output is what it was.  And a
C99 / C11 translation unit that calls the four new entries."""
import importlib
import json
import os
import subprocess

import numpy as np

import morph_cases as MC
from test_c_host_components import _write_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def test_a_c_host_calls_the_four_entries(tmp_path):
    src = tmp_path / "shape.c"
    src.write_text(
        '#include "maskrcnn_hip.h"\n'
        "int run(const uint32_t* counts, const int64_t* run_offsets, const int32_t* hs, const int32_t* ws, int64_t* measures, int64_t* offs, int64_t* areas2,\n"
        "        int64_t* obb, int32_t* xy)\n"
        "{\n"
        "    int64_t vertices = 0;\n"
        "    int64_t words[2 * MRCNN_MEASURE_WORDS];\n"
        "    int st = mrcnn_rle_measure_host(counts, run_offsets, 2, hs, ws, measures);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_rle_measure(counts, run_offsets, 2, hs, ws, MRCNN_HOST, words);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_rle_convex_hull_host(counts, run_offsets, 2, hs, ws, offs, NULL, NULL, NULL, &vertices, 0);\n"
        "    if (st != MRCNN_OK && st != MRCNN_ERR_SHAPE) return st;\n"
        "    if (vertices > 2 * MRCNN_HULL_LDS_COLUMNS) return MRCNN_ERR_SHAPE;\n"
        "    return mrcnn_rle_convex_hull(counts, run_offsets, 2, hs, ws, MRCNN_HOST, offs, areas2, obb, xy, &vertices, vertices);\n"
        "}\n")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def test_the_example_prints_and_writes_the_props(pkg, tmp_path):
    D = _mod("detection")
    libdir = os.path.dirname(_mod("_lib").SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_polygons.c")
    text = open(src).read()
    assert "mrcnn_rle_measure(" in text and "mrcnn_rle_convex_hull_host(" in text and "--props" in text
    exe = str(tmp_path / "maskrcnn_polygons")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--props"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "[--props]" in r.stderr

    a = MC.ellipse(40, 50, 20, 25, 9, 21); a[18:22, 20:30] = 0; a[2, 2] = 1                                  # a hole and a speck
    yy, xx = np.mgrid[0:40, 0:50]
    b = (np.abs(2 * (yy - 20) - (xx - 25)) <= 6).astype(np.uint8)                                            # a slanted bar
    c = np.zeros((30, 20), np.uint8); c[0:10, 0:10] = 1; c[25, 15] = 1
    d = np.zeros((30, 20), np.uint8)
    planes = [[a, b], [c, d]]
    sizes = [(40, 50), (30, 20)]
    f = tmp_path / "set.txt"
    _write_set(f, planes)
    rows = [[{"size": list(p.shape), "counts": MC.encode(p)} for p in row] for row in planes]

    def run(*flags):
        r = subprocess.run([exe, "--host", *flags, str(f)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [line.strip() for line in r.stdout.strip().splitlines()[1:]]

    def check(lines, want):
        """the props lines against rle_region_props_host: one per mask with a set pixel, in order"""
        kept = [k for k in range(4) if want["area"][k] > 0]
        assert len(lines) == len(kept)
        for line, k in zip(lines, kept):
            w = line.split()
            assert w[:3] == ["RLE", str(k), "props:"] and w[3::2][:3] == ["area", "perimeter", "centroid"], line
            assert int(w[4]) == int(want["area"][k]) and int(w[6]) == int(want["perimeter"][k])
            near = lambda got, ref: abs(float(got) - ref) <= 1e-9 * max(1.0, abs(ref))
            assert near(w[8], want["centroid"][k][0]) and near(w[9], want["centroid"][k][1]) and w[10] == "orientation" and near(w[11], want["orientation"][k]), line
            assert w[12] == "solidity" and near(w[13], want["solidity"][k]) and w[14] == "obb" and len(w) == 19, line
            corners = [[float(v) for v in pair.split(",")] for pair in w[15:]]
            assert all(near(g, r_) for got, ref in zip(corners, want["obb_corners"][k].tolist()) for g, r_ in zip(got, ref)), line

    plain = run()
    with_props = run("--props")
    assert with_props[:len(plain)] == plain and not any("props:" in line for line in plain)                 # the rings are what they were
    want = D.rle_region_props_host(rows, sizes)
    assert abs(want["orientation"][1]) > 0.3                                                                 # the bar is slanted
    check(with_props[len(plain):], want)
    filled = run("--fill-holes", "--props", "--min-area", "2")
    rings_then = [line for line in filled if "props:" not in line]
    cleaned = D.rle_remove_small_host(D.rle_fill_holes_host(rows, sizes), sizes, 2)
    want = D.rle_region_props_host(cleaned, sizes)
    assert int(want["area"][0]) == int(a.sum()) + 40 - 1 and len(rings_then) == 3
    check(filled[len(rings_then):], want)                                                                    # the final masks are measured
    geo = tmp_path / "out.geojson"
    run("--geojson", str(geo), "--props")
    features = json.loads(geo.read_text())["features"]
    want = D.rle_region_props_host(rows, sizes)
    assert [f_["properties"]["row"] for f_ in features] == [0, 1, 0]
    for f_, k in zip(features, (0, 1, 2)):
        p = f_["properties"]
        assert list(p) == ["image", "row", "area", "centroid", "orientation", "perimeter", "solidity", "obb"]
        assert p["perimeter"] == int(want["perimeter"][k]) and np.allclose(p["centroid"], want["centroid"][k], rtol=1e-9)
        assert np.allclose(p["obb"], want["obb_corners"][k], rtol=1e-9, atol=1e-9) and abs(p["orientation"] - want["orientation"][k]) < 1e-9
    run("--geojson", str(geo))
    assert all(list(f_["properties"]) == ["image", "row", "area"] for f_ in json.loads(geo.read_text())["features"])
    bad = tmp_path / "bad.txt"
    bad.write_text("1 1\n4 5 2 3 3\n")                          # sums to 6, the plane has 20: the library's text, the status as exit code
    r = subprocess.run([exe, "--host", "--props", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "rle_measure_host: RLE 0 sums to 6 pixels" in r.stderr, r.stderr
