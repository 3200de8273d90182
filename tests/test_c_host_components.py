"""examples/maskrcnn_polygons.c with --min-area and --fill-holes: built the way tests/test_c_host.py and tests/test_polygons_host.py
build it, run with --host (the definitions need no device) on a small set, and compared with the Python helpers; without the flags
its output is what it was.  And a C99 / C11 translation unit that calls the four new entries."""
import importlib
import os
import subprocess

import numpy as np

import morph_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def test_a_c_host_calls_the_four_entries(tmp_path):
    src = tmp_path / "components.c"
    src.write_text(
        '#include "maskrcnn_hip.h"\n'
        "int run(const uint32_t* counts, const int64_t* run_offsets, const int32_t* hs, const int32_t* ws, int64_t* offs, uint32_t* areas, int32_t* boxes,\n"
        "        uint8_t* flags, uint8_t* keep, uint32_t* out, int64_t* out_offs, int64_t* parent)\n"
        "{\n"
        "    int64_t out_n = 0;\n"
        "    int st = mrcnn_rle_components_host(counts, run_offsets, 2, hs, ws, 8, MRCNN_COMPONENTS_OF_ZEROS, offs, areas, boxes, flags, 64);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    st = mrcnn_rle_components(counts, run_offsets, 2, hs, ws, 4, MRCNN_COMPONENTS_OF_ONES, MRCNN_HOST, offs, NULL, NULL, NULL, 0);\n"
        "    if (st != MRCNN_OK && st != MRCNN_ERR_SHAPE) return st;\n"
        "    st = mrcnn_rle_components_select_host(counts, run_offsets, 2, hs, ws, 4, MRCNN_COMPONENTS_OF_ONES, keep, offs[2], MRCNN_COMPONENTS_SPLIT, out, 256,\n"
        "                                          out_offs, areas, boxes, parent, &out_n);\n"
        "    if (st != MRCNN_OK) return st;\n"
        "    return mrcnn_rle_components_select(counts, run_offsets, 2, hs, ws, 4, MRCNN_COMPONENTS_OF_ONES, keep, offs[2], MRCNN_COMPONENTS_MERGE, MRCNN_HOST,\n"
        "                                       out, 256, out_offs, NULL, NULL, NULL, &out_n);\n"
        "}\n")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


def _write_set(path, planes):
    """two images of one size each, `slots` RLEs per image, in the example's text layout"""
    lines = [f"{len(planes)} {len(planes[0])}"]
    for row in planes:
        lines.append(f"{row[0].shape[0]} {row[0].shape[1]}")
        for p in row:
            c = MC.encode(p)
            lines.append(f"{len(c)} " + " ".join(str(int(v)) for v in c))
    path.write_text("\n".join(lines) + "\n")


def test_the_example_filters_components_before_it_traces(pkg, tmp_path):
    D = _mod("detection")
    libdir = os.path.dirname(_mod("_lib").SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_polygons.c")
    text = open(src).read()
    assert "mrcnn_rle_components(" in text and "mrcnn_rle_components_select_host(" in text and "--min-area" in text and "--fill-holes" in text
    exe = str(tmp_path / "maskrcnn_polygons")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--min-area"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "--min-area A" in r.stderr and "--fill-holes" in r.stderr

    a = MC.ellipse(40, 50, 20, 25, 15, 20); a[18:22, 20:30] = 0; a[2, 2] = 1; a[37:39, 45:48] = 1            # a hole, a speck of 1, a speck of 6
    b = np.zeros((40, 50), np.uint8); b[5:30, 5:40] = 1; b[10:12, 10:12] = 0; b[20, 20] = 0
    c = np.zeros((30, 20), np.uint8); c[0:10, 0:10] = 1; c[3:6, 3:6] = 0; c[25, 15] = 1
    d = np.zeros((30, 20), np.uint8)
    planes = [[a, b], [c, d]]
    sizes = [(40, 50), (30, 20)]
    f = tmp_path / "set.txt"
    _write_set(f, planes)
    rows = [[{"size": list(p.shape), "counts": MC.encode(p)} for p in row] for row in planes]

    def lines_of(rles):
        rings, areas = D.rle_to_polygons_host(rles, sizes)
        out = []
        for b_ in range(2):
            for i in range(2):
                for r_, (ring, area) in enumerate(zip(rings[b_][i], areas[b_][i])):
                    out.append(f"RLE {2 * b_ + i} ring {r_} area {int(area)}: " + " ".join(f"{int(x)},{int(y)}" for x, y in ring))
        return out

    def run(*flags):
        r = subprocess.run([exe, "--host", *flags, str(f)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [line.strip() for line in r.stdout.strip().splitlines()[1:]]

    plain = run()
    assert plain == lines_of(rows) and sum(" area -" in line for line in plain) == 4                         # without the flags: what it was
    filled = run("--fill-holes")
    assert filled == lines_of(D.rle_fill_holes_host(rows, sizes)) and not any(" area -" in line for line in filled)
    cleaned = run("--min-area", "5")
    assert cleaned == lines_of(D.rle_remove_small_host(rows, sizes, 5)) and len(cleaned) == len(plain) - 2
    both = run("--min-area", "7", "--fill-holes")
    assert both == lines_of(D.rle_remove_small_host(D.rle_fill_holes_host(rows, sizes), sizes, 7)) and len(both) == 3
    assert run("--fill-holes", "--min-area", "7") == both                                                     # the two flags in either order
    bad = tmp_path / "bad.txt"
    bad.write_text("1 1\n4 5 2 3 3\n")                          # sums to 6, the plane has 20: the library's text, the status as exit code
    r = subprocess.run([exe, "--host", "--fill-holes", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "rle_components_host: RLE 0 sums to 6 pixels" in r.stderr, r.stderr
    geo = tmp_path / "out.geojson"
    with_geo = run("--tolerance", "0.5", "--geojson", str(geo), "--min-area", "7", "--fill-holes")
    assert len(with_geo) == 3 and geo.read_text().count('"Feature"') == 3
