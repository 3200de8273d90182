"""Measuring run-length masks, the host definitions (mrcnn_rle_measure_host, mrcnn_rle_convex_hull_host; detection.rle_measure_host,
rle_convex_hull_host, rle_region_props_host): the definitions against the rules restated in numpy and Python ints on dense planes
(tests/shape_cases.py), known answers, invariants against the tracer, the hole filler and the component splitter, every argument error
with its message and untouched outputs, the capacity protocol, the region properties against their formulas, and the GeoJSON
properties.  No test here needs a GPU."""
import ctypes as C
import decimal
import importlib
import json
import math
import os
import re

import numpy as np
import pytest

import shape_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SHAPE, INVALID = SC.SHAPE, SC.INVALID
Dec = decimal.Context(prec=50).create_decimal


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


@pytest.fixture(scope="module")
def cases():
    return SC.all_cases()


def test_symbols_declared_bound_and_exported():
    lib = _mod("_lib")
    L = lib.lib()
    header = open(os.path.join(INC, "maskrcnn_hip.h")).read()
    for name in ("mrcnn_rle_measure", "mrcnn_rle_measure_host", "mrcnn_rle_convex_hull", "mrcnn_rle_convex_hull_host"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes and f"MRCNN_API int {name}(" in header
    D = _mod("detection")
    m = re.search(r"#define\s+MRCNN_HULL_LDS_COLUMNS\s+(\d+)", header)
    assert m and int(m.group(1)) == lib.HULL_LDS_COLUMNS == D.HULL_LDS_COLUMNS
    m = re.search(r"#define\s+MRCNN_MEASURE_WORDS\s+(\d+)", header)
    assert m and int(m.group(1)) == lib.MEASURE_WORDS == 7
    for name in ("rle_measure", "rle_convex_hull", "rle_region_props"):
        assert callable(getattr(D, name)) and callable(getattr(D, name + "_host"))


# ---- 1. the definitions against the numpy rules ----------------------------------------------------------------------------------------------
def test_every_case_equals_the_numpy_rules(cases):
    """one ragged call per entry over all planes of all sizes"""
    names = cases["names"]
    assert len(names) == len(SC.SIZES) * len(SC.CONTENTS) and any((c[1:] == 0).any() for c in cases["runs"])       # zero-length runs are in
    want_m, want_rings, want_a2, want_box = SC.all_reference()
    counts, offs = SC.flat_set(cases["runs"])
    st, msg, m = SC.measure_host(counts, offs, cases["hs"], cases["ws"])
    assert st == 0, msg
    st, msg, ho, xy, a2, obb, nv = SC.hull_host(counts, offs, cases["hs"], cases["ws"])
    assert st == 0 and nv == int(ho[-1]) == len(xy), msg
    for k, name in enumerate(names):
        assert [int(v) for v in m[k]] == want_m[k], name
        ring = [tuple(p) for p in xy[int(ho[k]):int(ho[k + 1])].tolist()]
        assert ring == want_rings[k], name
        assert int(a2[k]) == want_a2[k] and obb[k].tolist() == want_box[k], name
        assert len(ring) == 0 if want_m[k][0] == 0 else len(ring) >= 4, name
    assert sum(len(r) > 12 for r in want_rings) > 10 and sum(len(r) == 0 for r in want_rings) >= len(SC.SIZES)


# ---- 2. known answers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (5, 12), (12, 5), (64, 64)])
def test_the_full_rectangle(h, w):
    D = _mod("detection")
    rows = [[{"size": [h, w], "counts": np.array([0, h * w], np.uint32)}]]
    m = D.rle_measure_host(rows)
    assert [int(v) for v in m[0]] == SC.full_measures(h, w) and int(m[0, 6]) == 2 * (h + w)
    hulls, a2, obb = D.rle_convex_hull_host(rows)
    assert hulls[0].tolist() == [[0, 0], [w, 0], [w, h], [0, h]] and int(a2[0]) == 2 * h * w
    assert obb[0].tolist() == [0, w, 0, 0, w * w, 0, w * h, 0]                       # a box on edge 0
    p = D.rle_region_props_host(rows)
    assert p["centroid"][0].tolist() == [w / 2, h / 2]
    c20 = (p["major_axis"][0] / 4) ** 2 if w >= h else (p["minor_axis"][0] / 4) ** 2
    c02 = (p["minor_axis"][0] / 4) ** 2 if w >= h else (p["major_axis"][0] / 4) ** 2
    assert abs(c20 - w * w / 12) <= 1e-12 * w * w and abs(c02 - h * h / 12) <= 1e-12 * h * h      # the covariance of a uniform rectangle
    if w > h:
        assert p["orientation"][0] == 0.0
    assert p["solidity"][0] == 1.0 and p["extent"][0] == 1.0 and p["hull_area"][0] == h * w
    assert p["obb_corners"][0].tolist() == [[0, 0], [w, 0], [w, h], [0, h]] and p["obb_size"][0].tolist() == [w, h] and p["obb_angle"][0] == 0.0


def test_the_diamonds_box_lies_on_edge_0():
    """a 45 degree diamond: all four hull edges of the staircase's hull give boxes of one area; the tie goes to edge 0"""
    r = 6
    yy, xx = np.mgrid[0:2 * r + 1, 0:2 * r + 1]
    P = (np.abs(yy - r) + np.abs(xx - r) <= r).astype(np.uint8)
    D = _mod("detection")
    hulls, a2, obb = D.rle_convex_hull_host([[{"size": list(P.shape), "counts": SC.encode(P)}]])
    ring = [tuple(p) for p in hulls[0].tolist()]
    assert ring == SC.hull_of(P) and len(ring) == 8
    want = SC.box_of(ring)
    assert obb[0].tolist() == want
    areas = []
    for e in range(8):
        dx, dy = ring[(e + 1) % 8][0] - ring[e][0], ring[(e + 1) % 8][1] - ring[e][1]
        d = [dx * x + dy * y for x, y in ring]; c = [dx * y - dy * x for x, y in ring]
        areas.append((max(d) - min(d)) * (max(c) - min(c)) / (dx * dx + dy * dy))
    assert areas.count(min(areas)) > 1 and areas.index(min(areas)) == int(obb[0, 0])         # several edges tie; the first of them is chosen


# ---- 3. invariants ---------------------------------------------------------------------------------------------------------------------------
def test_invariants_against_the_other_entries(cases):
    D = _mod("detection")
    pick = [k for k, name in enumerate(cases["names"]) if name.split("/")[1] in ("33x65", "63x31", "1100x9", "1x9")]
    rows = [[{"size": [int(cases["hs"][k]), int(cases["ws"][k])], "counts": cases["runs"][k]}] for k in pick]
    m = D.rle_measure_host(rows)
    hulls, a2, _obb = D.rle_convex_hull_host(rows)
    rings, _areas = D.rle_to_polygons_host(rows)
    filled = D.rle_fill_holes_host(rows)
    hulls_filled, a2_filled, _ = D.rle_convex_hull_host(filled)
    for j, k in enumerate(pick):
        name = cases["names"][k]
        length = sum(int(np.abs(np.diff(np.vstack([r, r[:1]]), axis=0)).sum()) for r in rings[j][0])
        assert int(m[j, 6]) == length, name                                          # the perimeter is the traced rings' edge length
        traced = {tuple(p) for r in rings[j][0] for p in np.asarray(r).tolist()}
        assert {tuple(p) for p in hulls[j].tolist()} <= traced, name                 # a hull vertex is a traced vertex
        assert int(a2[j]) >= 2 * int(m[j, 0]), name
        assert hulls_filled[j].tolist() == hulls[j].tolist() and int(a2_filled[j]) == int(a2[j]), name      # holes do not show in the hull
    parts, parent = D.rle_split_components_host(rows, None)
    pm = D.rle_measure_host([[p] for p in parts])
    summed = np.zeros_like(m)
    np.add.at(summed, parent, pm)
    assert (summed[:, :6] == m[:, :6]).all() and len(parts) > len(pick)              # the parts' moments sum to the whole's


# ---- 4. errors and the capacity protocol -----------------------------------------------------------------------------------------------------
def _four():
    planes = [SC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), SC.ellipse(20, 30, 12, 12, 5, 5), SC.ellipse(7, 5, 3, 2, 2, 1)]
    runs = [SC.encode(p) for p in planes]
    return planes, *SC.flat_set(runs), np.array([20, 7, 20, 7], np.int32), np.array([30, 5, 30, 5], np.int32)


def _raw(entry, counts, offs, n, hs, ws, capacity=64, memspace=0, nulls=()):
    """one of the four entries (a device entry with host pointers: argument errors need no device) with pre-filled outputs ->
    (status, message, buffers, n_vertices)"""
    L = _mod("_lib").lib()
    host = entry.endswith("_host")
    p = lambda name, a: None if name in nulls or a is None else a.ctypes.data
    keep = [np.ascontiguousarray(a) for a in (counts, offs, hs, ws)]
    head = (p("counts", keep[0]), p("run_offsets", keep[1]), n, p("heights", keep[2]), p("widths", keep[3])) + (() if host else (memspace,))
    nv = C.c_int64(77)
    if "measure" in entry:
        bufs = [np.full((max(1, n), 7), 77, np.int64)]
        st = getattr(L, "mrcnn_" + entry)(*head, p("measures", bufs[0]))
    else:
        bufs = [np.full(max(1, n) + 1, 77, np.int64), np.full(max(1, n), 77, np.int64), np.full((max(1, n), 8), 77, np.int64),
                np.full((max(1, capacity), 2), 77, np.int32)]
        st = getattr(L, "mrcnn_" + entry)(*head, p("hull_offsets", bufs[0]), p("hull_areas2", bufs[1]), p("obb", bufs[2]), p("xy", bufs[3]),
                                          None if "n_vertices" in nulls else C.byref(nv), capacity)
    return st, L.mrcnn_last_error().decode(), bufs, int(nv.value)


@pytest.mark.parametrize("entry", ["rle_measure_host", "rle_measure", "rle_convex_hull_host", "rle_convex_hull"])
def test_errors_and_untouched_outputs(entry):
    _planes, counts, offs, hs, ws = _four()

    def refused(code, text, **kw):
        args = dict(counts=counts, offs=offs, n=4, hs=hs, ws=ws)
        args.update(kw)
        st, msg, bufs, nv = _raw(entry, *(args[k] for k in ("counts", "offs", "n", "hs", "ws")), **{k: v for k, v in args.items() if k in ("capacity", "memspace", "nulls")})
        assert st == code and msg.startswith(entry + ":") and text in msg, (st, msg)
        assert all((b == 77).all() for b in bufs) and nv == 77, msg

    outputs = ("measures",) if "measure" in entry else ("hull_offsets", "n_vertices", "xy")
    for name in ("run_offsets", "heights", "widths", "counts") + outputs:
        refused(INVALID, "null", nulls=(name,))
    if not entry.endswith("_host"):
        refused(INVALID, "unknown memspace 7", memspace=7)
    if "hull" in entry:
        refused(INVALID, "vertex_capacity -1 is negative", capacity=-1)
    refused(SHAPE, "n -1 is negative", n=-1)
    for bad_side in (0, 32768):
        h2 = hs.copy(); h2[3] = bad_side
        refused(SHAPE, f"RLE 3 is {bad_side}x5: height and width must lie in 1..32767", hs=h2)
        w2 = ws.copy(); w2[1] = bad_side
        refused(SHAPE, f"RLE 1 is 7x{bad_side}", ws=w2)
    down = offs.copy(); down[2] = down[1] - 1
    refused(SHAPE, "run_offsets decrease at RLE 1", offs=down)
    if entry.endswith("_host"):                                  # (the device entries find a wrong total on the device: tests/test_gpu_rle_shape.py)
        bad = counts.copy()
        bad[int(offs[1]) + 1] += 3                               # RLE 1, and RLE 3 as well: the lowest is named
        bad[int(offs[3])] -= 1
        refused(SHAPE, "RLE 1 sums to 38 pixels, its 7x5 plane has 35", counts=bad)


def test_size_query_small_capacity_and_no_rles():
    _planes, counts, offs, hs, ws = _four()
    st, msg, want_offs, want_xy, want_a2, want_obb, need = SC.hull_host(counts, offs, hs, ws)
    assert st == 0 and need == int(want_offs[4]) >= 16, msg
    st, msg, bufs, nv = _raw("rle_convex_hull_host", counts, offs, 4, hs, ws, capacity=0, nulls=("xy",))            # the size query
    assert st == SHAPE and msg.startswith("rle_convex_hull_host:") and f"vertex_capacity >= {need}" in msg and nv == need
    assert bufs[0].tolist() == want_offs.tolist() and bufs[1].tolist() == want_a2.tolist() and (bufs[2] == want_obb).all()
    st, msg, bufs, nv = _raw("rle_convex_hull_host", counts, offs, 4, hs, ws, capacity=need - 1)
    assert st == SHAPE and f"holds {need - 1}: call again with vertex_capacity >= {need}" in msg and (bufs[3] == 77).all() and (bufs[2] == want_obb).all()
    st, msg, bufs, nv = _raw("rle_convex_hull_host", counts, offs, 4, hs, ws, capacity=need + 5)
    assert st == 0 and (bufs[3][:need] == want_xy).all() and (bufs[3][need:] == 77).all()
    L = _mod("_lib").lib()
    one, zero, nv = np.full(1, 77, np.int64), np.zeros(1, np.int64), C.c_int64(77)
    assert L.mrcnn_rle_convex_hull_host(None, zero.ctypes.data, 0, None, None, one.ctypes.data, None, None, None, C.byref(nv), 0) == 0      # n = 0
    assert one.tolist() == [0] and nv.value == 0
    assert L.mrcnn_rle_measure_host(None, zero.ctypes.data, 0, None, None, None) == 0


# ---- 5. the region properties ----------------------------------------------------------------------------------------------------------------
def test_region_props_follow_their_formulas():
    D = _mod("detection")
    planes = [SC.ellipse(60, 90, 28, 47, 14, 33), np.zeros((9, 9), np.uint8), SC.all_cases()["planes"][SC.all_cases()["names"].index("L/65x33")]]
    rows = [[{"size": list(P.shape), "counts": SC.encode(P)}] for P in planes]
    p = D.rle_region_props_host(rows)
    assert sorted(p) == sorted(D.REGION_PROPS) and all(len(v) == 3 for v in p.values())
    assert p["area"].tolist() == [int(P.sum()) for P in planes] and p["perimeter"][1] == 0 and p["hull_area"][1] == 0
    assert all(np.isnan(p[k][1]).all() for k in D.REGION_PROPS if k not in ("area", "perimeter", "hull_area"))
    for k in (0, 2):
        P = planes[k]
        ys, xs = np.nonzero(P)
        s1 = len(xs)
        cx, cy = xs.mean() + 0.5, ys.mean() + 0.5
        near = lambda got, want: abs(got - want) <= 1e-12 * max(1.0, abs(want))
        assert near(p["centroid"][k][0], cx) and near(p["centroid"][k][1], cy)
        # the formulas from the integers, in 50 decimal digits: what the float64 fields are held to, within 1e-12
        S1, Sx, Sy, Sxx, Sxy, Syy, _per = (Dec(v) for v in SC.measures_of(P))
        c20, c02, c11 = (S1 * Sxx - Sx * Sx) / (S1 * S1) + Dec(1) / 12, (S1 * Syy - Sy * Sy) / (S1 * S1) + Dec(1) / 12, (S1 * Sxy - Sx * Sy) / (S1 * S1)
        half, dev = (c20 + c02) / 2, (((c20 - c02) / 2) ** 2 + c11 ** 2).sqrt()
        l1, l2 = half + dev, half - dev
        assert near(p["major_axis"][k], float(4 * l1.sqrt())) and near(p["minor_axis"][k], float(4 * l2.sqrt()))
        assert near(p["orientation"][k], 0.5 * math.atan2(float(2 * c11), float(c20 - c02))) and near(p["eccentricity"][k], float((1 - l2 / l1).sqrt()))
        assert abs(float(c20) - (((xs - xs.mean()) ** 2).mean() + 1 / 12)) < 1e-9 * float(c20)       # (and the integers say what numpy says)
        m = SC.measures_of(P)
        ring = SC.hull_of(P)
        a2 = SC.area2_of(ring)
        assert near(p["compactness"][k], 4 * math.pi * s1 / m[6] ** 2) and near(p["hull_area"][k], a2 / 2) and near(p["solidity"][k], 2 * s1 / a2)
        assert near(p["extent"][k], s1 / ((xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)))
        e, dx, dy, dmin, dmax, cmin, cmax, _ = SC.box_of(ring)
        L2 = dx * dx + dy * dy
        corners = [((d * dx - c * dy) / L2, (d * dy + c * dx) / L2) for d, c in ((dmin, cmin), (dmax, cmin), (dmax, cmax), (dmin, cmax))]
        assert all(near(g, w) for got, want in zip(p["obb_corners"][k].tolist(), corners) for g, w in zip(got, want))
        assert near(p["obb_size"][k][0], (dmax - dmin) / math.sqrt(L2)) and near(p["obb_size"][k][1], (cmax - cmin) / math.sqrt(L2))
        assert near(p["obb_angle"][k], math.atan2(dy, dx)) and near(p["obb_center"][k][0], sum(c[0] for c in corners) / 4)
        twice = sum(corners[i][0] * corners[(i + 1) % 4][1] - corners[(i + 1) % 4][0] * corners[i][1] for i in range(4))
        assert twice > 0 and near(twice / 2, p["obb_size"][k][0] * p["obb_size"][k][1])          # clockwise on screen, and the rectangle's area
        for x, y in ring:                                        # the box holds the hull
            d, c = dx * x + dy * y, dx * y - dy * x
            assert dmin <= d <= dmax and cmin <= c <= cmax
    # the exact central moments against Python ints: an ellipse at the far corner of a large plane, where int64 products would wrap
    h = w = 30000
    P = SC.ellipse(1600, 1600, 800, 800, 700, 500)
    ys, xs = np.nonzero(P)
    xs, ys = xs.astype(np.int64) + (w - 1600), ys.astype(np.int64) + (h - 1600)
    pos = np.sort(xs * h + ys)
    starts = pos[np.concatenate(([True], np.diff(pos) > 1))]
    ends = pos[np.concatenate((np.diff(pos) > 1, [True]))] + 1
    counts = np.empty(2 * len(starts) + 1, np.int64)
    counts[0::2] = np.concatenate((starts, [h * w])) - np.concatenate(([0], ends))
    counts[1::2] = ends - starts
    q = D.rle_region_props_host([[{"size": [h, w], "counts": counts.astype(np.uint32)}]])
    small = D.rle_region_props_host([[{"size": [1600, 1600], "counts": SC.encode(P)}]])
    assert q["area"][0] == small["area"][0] and int(q["area"][0]) * int((xs * xs).sum()) > 2 ** 63
    for key in ("major_axis", "minor_axis", "orientation", "eccentricity", "obb_size", "obb_angle", "solidity", "compactness", "extent"):
        assert np.allclose(q[key], small[key], rtol=1e-9, atol=0), key                # a translation changes none of these
    assert np.allclose(q["centroid"][0] - small["centroid"][0], [w - 1600, h - 1600], rtol=0, atol=1e-9)


# ---- 6. GeoJSON ------------------------------------------------------------------------------------------------------------------------------
def test_geojson_gains_the_properties_only_when_asked():
    D, G = _mod("detection"), _mod("geojson")
    planes = [SC.ellipse(40, 60, 20, 30, 12, 22), SC.all_cases()["planes"][SC.all_cases()["names"].index("cross/33x65")][:, :60].copy()]
    planes[1] = np.pad(planes[1], ((0, 7), (0, 0)))
    rows = [[{"size": [40, 60], "counts": SC.encode(P)} for P in planes]]
    det = np.array([[[0.1, 0.1, 0.9, 0.9, 3, 0.8], [0.0, 0.0, 1.0, 1.0, 1, 0.6]]], np.float32)
    polygons = D.rle_to_polygons_host(rows, nest=True)
    props = D.rle_region_props_host(rows)
    kw = dict(sizes=[(40, 60)], transform=(0.5, 0.0, 100.0, 0.0, -0.5, 900.0))
    plain = G.dumps(det, polygons, None, **kw)
    assert G.dumps(det, polygons, None, props=None, **kw) == plain
    rich = json.loads(G.dumps(det, polygons, None, props=props, **kw))
    base = json.loads(plain)
    assert len(rich["features"]) == len(base["features"]) == 2
    for i, (f, g) in enumerate(zip(rich["features"], base["features"])):
        assert f["geometry"] == g["geometry"]
        keys = list(f["properties"])
        assert keys[:len(g["properties"])] == list(g["properties"]) and keys[len(g["properties"]):] == ["centroid", "orientation", "perimeter", "solidity", "obb"]
        assert all(f["properties"][k] == v for k, v in g["properties"].items())
        assert f["properties"]["centroid"] == props["centroid"][i].tolist() and f["properties"]["perimeter"] == int(props["perimeter"][i])
        assert f["properties"]["obb"] == [[0.5 * x + 100.0, -0.5 * y + 900.0] for x, y in props["obb_corners"][i].tolist()]
    with pytest.raises(ValueError):
        G.dumps(det, polygons, None, props={k: v[:1] for k, v in props.items()}, **kw)
