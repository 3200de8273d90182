"""Polygon rings nested into outlines and their holes, the parts that need no GPU: mrcnn_polygons_nest and its _host definition are
declared, listed, exported and bound; the definition equals the restatement of tests/nest_cases.py — connected components of the decoded
plane, which never looks at an edge — in parent, depth and the grouping, on every plane polygons_cases traces and on the planes made for
the nesting (concentric squares, two shells, diagonal contacts, a C with a blob in its mouth, a 40 x 41 checkerboard, a comb of 520
teeth, a ragged set with empty slots); the output has the properties the header states, on traced and on simplified rings; every
argument error is answered without a device through both entries; GeoJSON round-trips, fills back to the plane and is oriented; the C
example compiles and writes what json.loads reads."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nest_cases as NC
import polygons_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW_SYMBOLS = ("mrcnn_polygons_nest", "mrcnn_polygons_nest_host")
INVALID, HIP, SHAPE = NC.INVALID, NC.HIP, NC.SHAPE


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _det():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _gj():
    return importlib.import_module("mask-rcnn-coreml_amd.geojson")


@pytest.fixture(scope="module")
def nested(pkg):
    """every case once: (names, planes, the traced arrays, the host definition's nesting)"""
    cases = NC.all_cases()
    traced = PC.trace_host([r for _, r in cases])
    return [n for n, _ in cases], [NC.decode(r) for _, r in cases], traced, NC.nest_host(traced)


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
    assert len(L.mrcnn_polygons_nest.argtypes) == 12 and len(L.mrcnn_polygons_nest_host.argtypes) == 11
    assert len(L.mrcnn_rle_to_polygons.argtypes) == 15 and len(L.mrcnn_rle_to_polygons_host.argtypes) == 14       # the others keep theirs
    assert len(L.mrcnn_polygons_simplify.argtypes) == 11 and len(L.mrcnn_polygons_simplify_host.argtypes) == 10
    D = _det()
    assert callable(D.nest_polygons) and callable(D.nest_polygons_host) and callable(_gj().feature_collection) and callable(_gj().dumps)
    for word in ("probe(r)", "contains(q, r)", "OUTRANK", "nothing of the ring lies left of its start vertex", "forest", "nearest vertical edge",
                 "megapixel checkerboard", "nest first, then simplify"):
        assert word in hdr, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "nest_rule.h" in readme and "kernels_nest.hip" in readme and "mrcnn_polygons_nest" in readme and "geojson" in readme
    assert "mrcnn_polygons_nest" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "polygons_nest_ab.py" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "polygons_nest_ab.py"))
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("profiles", "README.md")):               # no template token is left in a document
        assert not re.search(r"\bNEST_[A-Z_]+\b", open(os.path.join(ROOT, doc)).read().replace("NEST_COORD_MAX", "")), doc


def test_c_hosts_compile_against_the_header(tmp_path):
    src = tmp_path / "nest.c"
    src.write_text(
        '#include "maskrcnn_hip.h"\n'
        "int run(const int64_t* rle_rings, int64_t n_rles, const int64_t* ring_offsets, const int32_t* xy, int64_t n_rings, int64_t* parent, int32_t* depth,\n"
        "        int64_t* rle_polys, int64_t* poly_rings, int64_t* ring_order)\n"
        "{\n"
        "    int64_t n = 0;\n"
        "    int st = mrcnn_polygons_nest_host(rle_rings, n_rles, ring_offsets, xy, n_rings, parent, depth, rle_polys, poly_rings, ring_order, &n);\n"
        "    if (st != MRCNN_OK || n > n_rings) return st;\n"
        "    return mrcnn_polygons_nest(rle_rings, n_rles, ring_offsets, xy, n_rings, MRCNN_HOST, parent, depth, rle_polys, poly_rings, ring_order, &n);\n"
        "}\n")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr


# ---- the definition against the restatement -------------------------------------------------------------------------------------
def test_the_definition_equals_the_restatement_on_every_case(nested):
    names, planes, traced, got = nested
    assert len(names) > 840 and traced["n_rings"] > 3500
    want = NC.restate(traced, planes)
    rr = traced["rle_rings"]
    for k, name in enumerate(names):                             # per case first: a difference is named
        r0, r1 = int(rr[k]), int(rr[k + 1])
        np.testing.assert_array_equal(got["parent"][r0:r1], want["parent"][r0:r1], err_msg=name)
        np.testing.assert_array_equal(got["depth"][r0:r1], want["depth"][r0:r1], err_msg=name)
    NC.assert_same(got, want, "all cases")
    assert got["parent"].dtype == np.int64 and got["depth"].dtype == np.int32


def test_the_output_has_the_stated_properties(nested):
    _names, _planes, traced, got = nested
    NC.assert_invariants(got, traced, traced=True)


def test_the_planes_meet_what_they_are_made_for(nested):
    names, _planes, traced, got = nested
    rr, ro = traced["rle_rings"], traced["ring_offsets"]

    def of(name):
        k = names.index(name)
        r0, r1 = int(rr[k]), int(rr[k + 1])
        p = got["parent"][r0:r1]
        return np.where(p >= 0, p - r0, -1), got["depth"][r0:r1], np.diff(ro[r0:r1 + 1]), int(got["rle_polys"][k + 1] - got["rle_polys"][k])

    parent, depth, _m, polys = of("concentric")
    assert sorted(depth.tolist()) == list(range(12)) and polys == 6                                   # one chain, depth 0 .. 11
    parent, depth, _m, polys = of("two_shells")
    assert sorted(depth.tolist()) == [0, 0, 1, 1, 1, 1, 2] and polys == 3                             # the island is a polygon of its own
    shells = np.nonzero(depth == 0)[0]
    assert [int((parent == s).sum()) for s in shells] == [2, 2] and depth[parent[np.nonzero(depth == 2)[0][0]]] == 1
    parent, depth, _m, polys = of("hole_with_island")
    assert depth.tolist() == [0, 1, 2, 3] and polys == 2
    parent, depth, _m, polys = of("island_diagonal_to_its_hole")
    assert sorted(depth.tolist()) == [0, 1, 2] and polys == 2
    parent, depth, _m, polys = of("hole_diagonal_to_the_outside")
    assert depth.tolist() == [0] and polys == 1                                                       # 8-connected to the cut corner: no hole at all
    parent, depth, _m, polys = of("c_shape")
    assert parent.tolist() == [-1, -1] and polys == 2                                                 # in the C's box, not in the C
    parent, depth, m, polys = of("checkerboard/40x41")
    assert len(m) == polys == 820 and (m == 4).all() and (parent == -1).all()                         # more than one block's worth of rings in one RLE
    parent, depth, m, polys = of("comb")
    assert m[0] > 2048 and len(m) == 521 and polys == 1 and (parent[1:] == 0).all() and (m[1:] == 4).all()


def test_a_ragged_set_with_empty_slots(pkg):
    rows, sizes, planes = NC.ragged_set()
    flat = [r for row in rows for r in row]
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    traced = PC.trace_host(flat, n_images=3, slots=4, hs=hs, ws=ws)
    got = NC.nest_host(traced)
    NC.assert_same(got, NC.restate(traced, planes), "ragged")
    NC.assert_invariants(got, traced)
    per_rle = np.diff(got["rle_polys"])
    assert per_rle.tolist() == [0, 3, 0, 3, 2, 0, 0, 1, 6, 0, 6, 0]                                  # equal neighbours at both ends and in the middle
    assert (got["parent"] >= int(traced["rle_rings"][3])).sum() > 10                                  # global indices, not local ones
    # the Python forms on the same set: flat and nested say the same
    D = _det()
    nested_rings = D.rle_to_polygons_host(rows, sizes)
    N = D.nest_polygons_host(nested_rings)
    NC.assert_same(D.nest_polygons_host(nested_rings, flat=True), got, "nested in, flat out")
    NC.assert_same(D.nest_polygons_host(D.rle_to_polygons_host(rows, sizes, flat=True)), got, "flat in")
    k = 0
    for b in range(3):
        for i in range(4):
            r0 = int(traced["rle_rings"][k])
            want = [[int(r) - r0 for r in got["ring_order"][got["poly_rings"][p]:got["poly_rings"][p + 1]]] for p in range(got["rle_polys"][k], got["rle_polys"][k + 1])]
            assert N["nest"][b][i] == want and len(N["parent"][b][i]) == len(N["depth"][b][i]) == len(nested_rings[0][b][i])
            assert all(-1 <= p < len(nested_rings[0][b][i]) for p in N["parent"][b][i])
            k += 1


# ---- general integer rings --------------------------------------------------------------------------------------------------------
def _rule_in_python(arrays):
    """parent by the header's words on any integer rings, in numpy int64: per candidate q, every probe of its RLE at once"""
    rr, ro, xy = arrays["rle_rings"], arrays["ring_offsets"], arrays["xy"].astype(np.int64)
    R = len(ro) - 1
    area2 = np.zeros(R, np.int64)
    for r in range(R):
        v = xy[ro[r]:ro[r + 1]]
        area2[r] = int((v[:, 0] * np.roll(v[:, 1], -1) - np.roll(v[:, 0], -1) * v[:, 1]).sum()) if len(v) else 0
    size = np.abs(area2)
    parent = np.full(R, -1, np.int64)
    for k in range(len(rr) - 1):
        mine = [r for r in range(int(rr[k]), int(rr[k + 1])) if ro[r + 1] > ro[r]]
        if not mine:
            continue
        PX, PY = 2 * xy[ro[mine], 0] + 1, 2 * xy[ro[mine], 1] + 1                                    # the probes, doubled
        best = {r: None for r in mine}
        for q in range(int(rr[k]), int(rr[k + 1])):
            v = 2 * xy[ro[q]:ro[q + 1]]
            if len(v) < 3:
                continue
            a, b = v[:, None, :], np.roll(v, -1, axis=0)[:, None, :]
            straddles = (a[..., 1] < PY[None, :]) != (b[..., 1] < PY[None, :])
            dy = b[..., 1] - a[..., 1]
            # the edge's x on the probe's line, times dy, against the probe's x times dy: the inequality turns with the sign of dy
            lhs, rhs = a[..., 0] * dy + (b[..., 0] - a[..., 0]) * (PY[None, :] - a[..., 1]), PX[None, :] * dy
            left = np.where(dy > 0, lhs < rhs, lhs > rhs)
            inside = (straddles & left).sum(0) % 2 == 1
            for j, r in enumerate(mine):
                if r == q or not inside[j] or not (size[q] > size[r] or (size[q] == size[r] and q < r)):
                    continue
                if best[r] is None or (size[q], q) < (size[best[r]], best[r]):
                    best[r] = q
        for r in mine:
            parent[r] = -1 if best[r] is None else best[r]
    return parent, size


def test_simplified_rings_nest_into_a_forest_that_indexes_them_one_for_one(nested):
    names, _planes, traced, got = nested
    D = _det()
    simple = D.simplify_polygons_host(traced, 2.0)
    assert simple["n_rings"] == traced["n_rings"] and simple["n_vertices"] < traced["n_vertices"]
    np.testing.assert_array_equal(simple["rle_rings"], traced["rle_rings"])                           # one for one: the traced nesting indexes them
    assert (np.diff(simple["ring_offsets"]) < 3).any()                                                # general rings: some contain nothing any more
    N = NC.nest_host(simple)
    NC.assert_invariants(N, simple, traced=False)
    parent, size = _rule_in_python(simple)
    np.testing.assert_array_equal(N["parent"], parent)
    has = N["parent"] >= 0
    q, r = N["parent"][has], np.nonzero(has)[0]
    assert ((size[q] > size[r]) | ((size[q] == size[r]) & (q < r))).all()                             # the strict order: no cycle is possible
    np.testing.assert_array_equal(size, np.abs(simple["areas2"]))
    # and the same restatement of the rule on the traced rings
    np.testing.assert_array_equal(_rule_in_python(traced)[0], got["parent"])


def test_hand_made_rings_ties_and_rings_without_vertices(pkg):
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    rings = [sq(0, 0, 8, 8), [(0, 0), (0, 8), (8, 8), (8, 0)], [], sq(2, 2, 6, 6), [(3, 3)], [(3, 3), (5, 5)], sq(0, 0, 8, 8), [(1, 1), (7, 1), (1, 7)]]
    ro = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    xy = np.array([p for r in rings for p in r], np.int32).reshape(-1, 2)
    arrays = {"rle_rings": np.array([0, len(rings)], np.int64), "ring_offsets": ro, "xy": xy}
    N = NC.nest_host(arrays)
    # Three copies of one square, 0, 1 (the other way round) and 6: among equal |area2| the smaller index outranks, and of the equal rings
    # that contain a probe the smallest index is the parent, so 1 and 6 are both children of 0 and so is the triangle 7 (|area2| 36 against
    # 128).  The inner square 3 (32) lies in the triangle, the rings of one and two vertices in the inner square; the empty ring 2 has no
    # probe and no parent.
    assert N["parent"].tolist() == [-1, 0, -1, 7, 3, 3, 0, 0], N["parent"]
    assert N["depth"].tolist() == [0, 1, 0, 2, 3, 3, 1, 1]
    NC.assert_invariants(N, arrays, traced=False)
    np.testing.assert_array_equal(_rule_in_python(arrays)[0], N["parent"])
    # A probe ON an edge is not left of it.  The triangle's left side x + y = 8 passes through (3.5, 4.5), the probe of ring 1: that side
    # is no crossing and the side x = 7 lies right of the probe, none in all, not contained.  Ring 2's probe (4.5, 4.5) has the side at 3.5.
    rings = [[(7, 1), (7, 7), (1, 7)], [(3, 4), (4, 4), (4, 5)], [(4, 4), (5, 4), (5, 5)]]
    ro = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    arrays = {"rle_rings": np.array([0, 3], np.int64), "ring_offsets": ro, "xy": np.array([p for r in rings for p in r], np.int32)}
    assert NC.nest_host(arrays)["parent"].tolist() == [-1, -1, 0]


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def _few():
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    rings = [sq(0, 0, 9, 9), sq(1, 1, 4, 4)[::-1], sq(20, 0, 25, 5), sq(0, 0, 3, 3)]
    ro = np.concatenate(([0], np.cumsum([len(r) for r in rings]))).astype(np.int64)
    return np.array([0, 2, 2, 3, 4], np.int64), ro, np.array([p for r in rings for p in r], np.int32)


@pytest.mark.parametrize("entry", NEW_SYMBOLS[::-1])
def test_argument_errors_need_no_device(pkg, entry):
    rr, ro, xy = _few()
    who = entry[len("mrcnn_"):]
    for kw in [dict(null=(name,)) for name in ("rle_rings", "ring_offsets", "xy", "parent", "depth", "rle_polys", "poly_rings", "ring_order", "n_polys")] + \
              [dict(n_rles=-1), dict(n_rings=-1)]:
        st, msg, out = NC.call(entry, rr, ro, xy, **kw)
        assert st == INVALID and msg.startswith(who + ":"), (kw, st, msg)
        assert all((out[k] == -9).all() for k in NC.KEYS) and out["n_polys"] == -9, kw
    if entry == "mrcnn_polygons_nest":
        st, msg, out = NC.call(entry, rr, ro, xy, memspace=7)
        assert st == INVALID and "memspace" in msg and all((out[k] == -9).all() for k in NC.KEYS), msg
    else:
        st, msg, out = NC.call(entry, rr, ro, xy)
        assert st == 0 and out["n_polys"] == 3 and out["parent"].tolist() == [-1, 0, -1, -1], msg
        st, msg, out = NC.call(entry, np.zeros(4, np.int64), np.zeros(1, np.int64), np.zeros((0, 2), np.int32), null=("xy", "parent", "depth", "ring_order"))
        assert st == 0 and out["n_polys"] == 0 and out["rle_polys"].tolist() == [0, 0, 0, 0] and out["poly_rings"][0] == 0, msg      # n_rings = 0 is legal


@pytest.mark.parametrize("entry", NEW_SYMBOLS[::-1])
def test_a_bad_array_is_named_and_nothing_is_written(pkg, entry):
    rr, ro, xy = _few()
    xy = xy.reshape(-1, 2)
    at = int(ro[2]) + 1                                          # a vertex of ring 2
    edit = lambda a, i, v: np.concatenate((a[:i], [v], a[i + 1:])).astype(a.dtype)
    low, high = xy.copy(), xy.copy()
    low[at, 0], high[at, 1] = -1, 32768
    wide = np.array([0, 1 << 31], np.int64)
    for r_, o_, v_, n_rings, needle in (
            (rr, ro, low, None, "ring 2 has a coordinate outside 0..32767"), (rr, ro, high, None, "ring 2 has a coordinate outside 0..32767"),
            (rr, edit(ro, 4, ro[3] - 2), xy, None, "at ring 3"), (rr, ro - 1, xy, None, "at ring 0"),
            (np.array([0, 1], np.int64), wide, xy, None, "span 2^31 vertices or more at ring 0"),
            (edit(rr, 0, 1), ro, xy, None, "at RLE 0"), (edit(rr, 2, 1), ro, xy, None, "at RLE 1"), (edit(rr, 4, 3), ro, xy, None, "at RLE 3"),
            (edit(rr, 4, 5), ro, xy, None, "n_rings = 4 at RLE 3")):
        st, msg, out = NC.call(entry, r_, o_, v_, n_rings=n_rings)
        assert st == SHAPE and needle in msg and msg.startswith(entry[len("mrcnn_"):] + ":"), (needle, st, msg)
        assert all((out[k] == -9).all() for k in NC.KEYS) and out["n_polys"] == -9, needle
    st, msg, out = NC.call(entry, np.zeros(1, np.int64), ro, xy, n_rles=0)                            # rings, and no RLE to own them
    assert st == SHAPE and "at RLE 0" in msg, msg


def test_no_cpu_fallback_without_a_gpu(pkg):
    import torch
    lib = _lib()
    D = _det()
    rr, ro, xy = _few()
    flat = {"rle_rings": rr, "ring_offsets": ro, "xy": xy.reshape(-1, 2)}
    want = D.nest_polygons_host(flat)
    assert want["n_polys"] == 3 and want["parent"].tolist() == [-1, 0, -1, -1]
    if torch.cuda.is_available():                                # with a device the two agree; without one there is no quiet way round
        NC.assert_same(D.nest_polygons(flat), want)
        return
    for call in (lambda: D.nest_polygons(flat), lambda: D.rle_to_polygons([[dict(PC.cases())["full"]]], nest=True)):
        with pytest.raises(lib.MrcnnError) as e:
            call()
        assert e.value.code == HIP


# ---- the Python surface and GeoJSON ----------------------------------------------------------------------------------------------------
def _small_rows():
    """the small planes as one image each, one slot: (rows, sizes, planes, det_src)"""
    c = dict(NC.all_cases())
    rows = [[c[name]] for name in NC.SMALL]
    sizes = [tuple(int(v) for v in r[0]["size"]) for r in rows]
    det = np.zeros((len(rows), 1, 6), np.float32)
    det[:, 0, :4] = [0, 0, 1, 1]
    det[:, 0, 4] = 2
    det[:, 0, 5] = 0.5 + 0.01 * np.arange(len(rows))
    return rows, sizes, [NC.decode(r[0]) for r in rows], det


def _inside(ring, h, w):
    """the pixel centres of an h x w plane inside a closed ring of GeoJSON positions, even-odd"""
    py, px = np.mgrid[0:h, 0:w] + 0.5
    inside = np.zeros((h, w), bool)
    for (ax, ay), (bx, by) in zip(ring, ring[1:]):
        if ay == by:
            continue
        hit = ((ay <= py) != (by <= py)) & (px < ax + (py - ay) * (bx - ax) / (by - ay))
        inside ^= hit
    return inside


def _fill(feature, h, w, to_pixels=lambda p: p):
    g = feature["geometry"]
    polys = [g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]
    assert g["type"] in ("Polygon", "MultiPolygon") and (len(polys) > 1) == (g["type"] == "MultiPolygon")
    plane = np.zeros((h, w), bool)
    for poly in polys:
        mine = _inside([to_pixels(p) for p in poly[0]], h, w)
        for hole in poly[1:]:
            mine &= ~_inside([to_pixels(p) for p in hole], h, w)
        plane |= mine
    return plane


def _shoelace(ring):
    return sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(ring, ring[1:]))


def test_rle_to_polygons_returns_the_nesting_of_the_traced_rings(pkg):
    D = _det()
    rows, sizes, _planes, _det_src = _small_rows()
    plain = D.rle_to_polygons_host(rows, sizes)
    assert len(plain) == 2                                       # nest=False: today's result, exactly
    want = D.nest_polygons_host(plain)
    for tol in (None, 1.0):
        rings, areas, N = D.rle_to_polygons_host(rows, sizes, tolerance=tol, nest=True)
        assert N["nest"] == want["nest"] and all(np.array_equal(a, c) for x, y in zip(N["parent"], want["parent"]) for a, c in zip(x, y))
        flat = D.rle_to_polygons_host(rows, sizes, flat=True, tolerance=tol, nest=True)
        NC.assert_same(flat["nest"], D.nest_polygons_host(D.rle_to_polygons_host(rows, sizes, flat=True)), f"tolerance {tol}")
    assert sum(len(r) for row in rings for rle in row for r in rle) < sum(len(r) for row in plain[0] for rle in row for r in rle)


@pytest.mark.parametrize("flip", [False, True])
def test_geojson_fills_back_to_the_plane_and_is_oriented(pkg, flip):
    D, G = _det(), _gj()
    rows, sizes, planes, det = _small_rows()
    polygons = D.rle_to_polygons_host(rows, sizes, nest=True)
    H = 40
    transform = (0.5, 0.0, 100.0, 0.0, -0.5, float(H)) if flip else None                              # y up, half-pixel units, an offset
    back = (lambda p: ((p[0] - 100.0) / 0.5, (p[1] - H) / -0.5)) if flip else (lambda p: p)
    names = [f"class {i}" for i in range(4)]
    data = G.dumps(det, polygons, None, sizes=sizes, class_names=names, transform=transform, image_ids=[f"im{b}" for b in range(len(rows))])
    assert isinstance(data, bytes) and data == G.dumps(det, polygons, None, sizes=sizes, class_names=names, transform=transform,
                                                       image_ids=[f"im{b}" for b in range(len(rows))])
    fc = json.loads(data)
    assert fc == json.loads(json.dumps(G.feature_collection(det, polygons, None, sizes=sizes, class_names=names, transform=transform,
                                                            image_ids=[f"im{b}" for b in range(len(rows))])))
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == len(rows) - 0
    multi = holes = 0
    for b, f in enumerate(fc["features"]):
        h, w = sizes[b]
        p = f["properties"]
        assert f["type"] == "Feature" and list(p) == ["image", "row", "category_id", "category", "score", "bbox", "area"]
        assert p["image"] == f"im{b}" and p["row"] == 0 and p["category_id"] == 2 and p["category"] == "class 2" and p["area"] == int(planes[b].sum())
        assert p["bbox"] == [0.0, 0.0, float(w), float(h)] and abs(p["score"] - float(det[b, 0, 5])) < 1e-7
        np.testing.assert_array_equal(_fill(f, h, w, back), planes[b] != 0, err_msg=NC.SMALL[b])
        g = f["geometry"]
        for poly in ([g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]):
            for j, ring in enumerate(poly):
                assert ring[0] == ring[-1] and len(ring) >= 5 and (_shoelace(ring) > 0) == (j == 0), (NC.SMALL[b], j)
            holes += len(poly) - 1
        multi += g["type"] == "MultiPolygon"
    assert multi >= 4 and holes >= 10


def test_geojson_drops_small_shells_with_their_holes_and_degenerate_rings(pkg):
    D, G = _det(), _gj()
    rows, sizes, planes, det = _small_rows()
    b = NC.SMALL.index("two_shells")
    one = ([rows[b]], [sizes[b]], det[b:b + 1])
    polygons = D.rle_to_polygons_host(one[0], one[1], nest=True)
    full = G.feature_collection(one[2], polygons, None)["features"][0]
    assert full["geometry"]["type"] == "MultiPolygon" and [len(p) for p in full["geometry"]["coordinates"]] == [3, 1, 3]
    assert full["properties"]["bbox"] == [1.0, 1.0, 22.0, 10.0] and "category" not in full["properties"]         # no sizes: the shells' box
    # the island has 4 pixels: min_area 5 drops it alone; 101 drops both 10 x 10 shells, and their holes go along
    fewer = G.feature_collection(one[2], polygons, None, min_area=5)["features"][0]
    assert [len(p) for p in fewer["geometry"]["coordinates"]] == [3, 3] and fewer["properties"]["area"] == full["properties"]["area"]
    assert G.feature_collection(one[2], polygons, None, min_area=101)["features"] == []
    assert json.loads(G.dumps(one[2], polygons, None, min_area=101)) == {"type": "FeatureCollection", "features": []}
    # a row without a score is no detection
    assert G.feature_collection(np.zeros_like(one[2]), polygons, None)["features"] == []
    # simplified until rings degenerate: a shell of 2 vertices goes with its holes, a hole of 2 vertices alone
    rings, areas, N = polygons
    cut = [[[r if j not in (1, 4) else r[:2] for j, r in enumerate(rings[0][0])]]]
    groups = N["nest"][0][0]
    gone = G.feature_collection(one[2], (cut, areas), N)["features"][0]["geometry"]["coordinates"]
    want = [1 + sum(1 for hh in g[1:] if hh not in (1, 4)) for g in groups if g[0] not in (1, 4)]
    assert [len(p) for p in gone] == want and sum(want) < 7
    with pytest.raises(ValueError):
        G.feature_collection(one[2], polygons[:2], None)


# ---- the C example -----------------------------------------------------------------------------------------------------------------
def test_the_example_writes_geojson_and_prints_what_it_printed(pkg, tmp_path):
    libdir = os.path.dirname(_lib().SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_polygons.c")
    text = open(src).read()
    assert "mrcnn_polygons_nest(" in text and "mrcnn_polygons_nest_host(" in text
    exe = str(tmp_path / "maskrcnn_polygons")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--host", "--geojson", "x.json"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "--geojson" in r.stderr
    c = dict(NC.all_cases())
    rles = [c["two_shells"], c["hole_with_island"], c["empty"]]
    planes = [NC.decode(r) for r in rles]
    f = tmp_path / "set.txt"
    f.write_text("3 1\n" + "".join("%d %d %d\n%s\n" % (r["size"][0], r["size"][1], len(r["counts"]), " ".join(str(int(v)) for v in r["counts"])) for r in rles))
    plain = subprocess.run([exe, "--host", str(f)], capture_output=True, timeout=60)
    assert plain.returncode == 0, plain.stderr
    lines = plain.stdout.decode().splitlines()                   # without the flag: the lines of the tracer's rings, as they always were
    tr = PC.trace_host(rles)
    want = ["%d rings, %d vertices in 3 x 1 RLEs" % (tr["n_rings"], tr["n_vertices"])]
    for k in range(3):
        rings, areas = PC.rings_of(tr, k)
        want += ["RLE %d ring %d area %d: %s" % (k, j, int(a), " ".join(f"{x},{y}" for x, y in ring)) for j, (ring, a) in enumerate(zip(rings, areas))]
    assert lines == want and plain.stdout.endswith(b"\n")
    out = tmp_path / "out.geojson"
    r = subprocess.run([exe, "--host", "--geojson", str(out), str(f)], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == plain.stdout, r.stderr
    fc = json.loads(out.read_text())
    assert fc["type"] == "FeatureCollection" and [ft["properties"] for ft in fc["features"]] == [
        {"image": 0, "row": 0, "area": int(planes[0].sum())}, {"image": 1, "row": 0, "area": int(planes[1].sum())}]     # the empty mask has no Feature
    assert [ft["geometry"]["type"] for ft in fc["features"]] == ["MultiPolygon", "MultiPolygon"]
    for ft, plane in zip(fc["features"], planes):
        np.testing.assert_array_equal(_fill(ft, *plane.shape), plane != 0)
        for poly in ft["geometry"]["coordinates"]:
            assert all(ring[0] == ring[-1] and (_shoelace(ring) > 0) == (j == 0) for j, ring in enumerate(poly))
    # with a tolerance the nesting stays the traced rings' and the file still parses
    r = subprocess.run([exe, "--host", "--tolerance", "1", "--geojson", str(out), str(f)], capture_output=True, timeout=60)
    assert r.returncode == 0 and len(json.loads(out.read_text())["features"]) == 2, r.stderr
