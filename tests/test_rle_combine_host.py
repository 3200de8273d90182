"""The set algebra of run-length masks, the host definition (mrcnn_rle_combine_host; detection.rle_combine_host and its helpers): the
definition against the rule restated in numpy on dense planes (tests/combine_cases.py), identities, every argument error with its
message and untouched outputs, the capacity protocol, rle_disjoint_host against instance_map_rle_host, the union of the parts
rle_split_components_host cuts, and a C program over the header.  No test here needs a GPU."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import combine_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SHAPE, INVALID = CC.SHAPE, CC.INVALID


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


@pytest.fixture(scope="module")
def cases():
    return CC.all_cases()


def test_symbols_declared_bound_and_exported():
    lib = _mod("_lib")
    L = lib.lib()
    header = open(os.path.join(INC, "maskrcnn_hip.h")).read()
    for name in ("mrcnn_rle_combine", "mrcnn_rle_combine_host"):
        assert name in lib.EXPORTED_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes and f"MRCNN_API int {name}(" in header
    assert (lib.RLE_OR, lib.RLE_AND, lib.RLE_XOR, lib.RLE_DIFF) == (0, 1, 2, 3)
    for k, name in enumerate(("MRCNN_RLE_OR", "MRCNN_RLE_AND", "MRCNN_RLE_XOR", "MRCNN_RLE_DIFF")):
        assert f"#define {name} {k}\n" in header
    D = _mod("detection")
    for name in ("rle_combine", "rle_union", "rle_intersection", "rle_xor", "rle_difference", "rle_disjoint"):
        assert callable(getattr(D, name)) and callable(getattr(D, name + "_host"))


# ---- 1. the definition against the numpy rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(CC.OPS))
def test_every_case_equals_the_numpy_rule(cases, op):
    """one ragged call over all groups; out_counts, out_run_offsets, areas and bboxes_xywh against the planes of the restatement"""
    from morph_cases import stats
    code = CC.OPS[op]
    groups, names = cases["groups"], cases["names"]
    assert 200 < len(groups) < 1000 and "g100/33x65" in names and max(len(g) for g in groups) == 100
    assert any((c[1:] == 0).any() for c in cases["runs"])                           # zero-length runs are in
    assert any(len(set(g)) < len(g) for g in groups) and len({(h, w) for h, w in zip(cases["hs"], cases["ws"])}) == len(CC.SIZES)
    st, msg, out, offs, areas, boxes = CC.combine_host(*CC.flat_set(cases["runs"]), cases["hs"], cases["ws"], *CC.flat_groups(groups), code)
    assert st == 0, msg
    empties = fulls = 0
    for g, (name, idx) in enumerate(zip(names, groups)):
        want = CC.reference([cases["planes"][k] for k in idx], code)
        got = out[int(offs[g]):int(offs[g + 1])]
        assert got.tolist() == CC.encode(want).tolist(), (op, name)
        assert (int(areas[g]), boxes[g].tolist()) == stats(want), (op, name)
        assert (got[1:] > 0).all(), (op, name)                                      # canonical: only counts[0] may be 0
        empties += want.sum() == 0
        fulls += bool(want.all())
    assert empties > 0 and fulls > 0


def test_the_ellipses_of_the_cases_overlap_and_do_not(cases):
    base = [k for k, (h, w) in enumerate(zip(cases["hs"], cases["ws"])) if (h, w) == (130, 40)][0]
    a, b, c = (cases["planes"][base + CC.POOL.index(n)] for n in ("ellipse_a", "ellipse_b", "ellipse_c"))
    assert (a & b).any() and not (a & c).any() and c.any()


def _pairwise(cases, op):
    """rand0 op rand1 on every plane -> the planes"""
    D = _mod("detection")
    out = []
    for h, w in CC.SIZES:
        base = [k for k, (h_, w_) in enumerate(zip(cases["hs"], cases["ws"])) if (h_, w_) == (h, w)][0]
        a, b = (cases["runs"][base + CC.POOL.index(n)] for n in ("rand0", "rand1"))
        rows = [[{"size": [h, w], "counts": a}, {"size": [h, w], "counts": b}]]
        r, areas, _ = D.rle_combine_host(rows, None, [[0, 1]], op)
        out.append((CC.decode(r[0]["counts"], h, w), int(areas[0]), rows))
    return out


def test_identities_on_the_random_planes(cases):
    D = _mod("detection")
    union, inter, xor = (_pairwise(cases, op) for op in ("or", "and", "xor"))
    for (u, au, rows), (i, ai, _), (x, _ax, _) in zip(union, inter, xor):
        h, w = rows[0][0]["size"]
        a, b = (CC.decode(e["counts"], h, w) for e in rows[0])
        assert au + ai == int(a.sum()) + int(b.sum())                               # |A u B| + |A n B| = |A| + |B|
        both = [[{"size": [h, w], "counts": CC.encode(u)}, {"size": [h, w], "counts": CC.encode(i)}]]
        d, _, _ = D.rle_combine_host(both, None, [[0, 1]], "diff")
        assert d[0]["counts"].tolist() == CC.encode(x).tolist()                     # A xor B = (A u B) diff (A n B)
        e, area, box = D.rle_combine_host(rows, None, [[0, 0], [1, 1]], "diff")     # A diff A is empty
        assert [r["counts"].tolist() for r in e] == [[h * w]] * 2 and area.tolist() == [0, 0] and not box.any()


# ---- 2. errors, capacity -------------------------------------------------------------------------------------------------------------------
def _three():
    from morph_cases import ellipse
    planes = [ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), ellipse(20, 30, 12, 12, 5, 5), ellipse(7, 5, 3, 2, 2, 1)]
    runs = [CC.encode(p) for p in planes]
    return planes, *CC.flat_set(runs), np.array([20, 7, 20, 7], np.int32), np.array([30, 5, 30, 5], np.int32)


GROUPS = [[0, 2], [1, 3], [2, 0, 2]]


def _raw(entry_host, counts, offs, n, hs, ws, goffs, mem, G, op, capacity=64, memspace=0, nulls=()):
    """either entry (the device entry with host pointers: argument errors need no device) with pre-filled outputs ->
    (status, message, [out_counts, out_run_offsets, areas, bboxes])"""
    lib = _mod("_lib")
    L = lib.lib()
    bufs = [np.full(max(1, capacity), 77, np.uint32), np.full(max(1, G) + 1, 77, np.int64), np.full(max(1, G), 77, np.uint32), np.full((max(1, G), 4), 77, np.int32)]
    p = lambda name, a: None if name in nulls or a is None else np.ascontiguousarray(a).ctypes.data
    keep = [np.ascontiguousarray(a) for a in (counts, offs, hs, ws, goffs, mem)]
    head = (p("counts", keep[0]), p("run_offsets", keep[1]), n, p("heights", keep[2]), p("widths", keep[3]), p("group_offsets", keep[4]), p("members", keep[5]), G, op)
    tail = (p("out_counts", bufs[0]), capacity, p("out_run_offsets", bufs[1]), p("areas", bufs[2]), p("bboxes", bufs[3]))
    st = L.mrcnn_rle_combine_host(*head, *tail) if entry_host else L.mrcnn_rle_combine(*head, memspace, *tail)
    return st, L.mrcnn_last_error().decode(), bufs


@pytest.mark.parametrize("entry_host", [True, False], ids=["rle_combine_host", "rle_combine"])
def test_errors_and_untouched_outputs(entry_host):
    who = "rle_combine_host:" if entry_host else "rle_combine:"
    _planes, counts, offs, hs, ws = _three()
    goffs, mem = CC.flat_groups(GROUPS)
    i64 = lambda a: np.array(a, np.int64)

    def refused(code, text, **kw):
        args = dict(counts=counts, offs=offs, n=4, hs=hs, ws=ws, goffs=goffs, mem=mem, G=3, op=CC.OR)
        args.update(kw)
        st, msg, bufs = _raw(entry_host, *(args[k] for k in ("counts", "offs", "n", "hs", "ws", "goffs", "mem", "G", "op")),
                             **{k: v for k, v in args.items() if k in ("capacity", "memspace", "nulls")})
        assert st == code and msg.startswith(who) and text in msg, (st, msg)
        assert all((b == 77).all() for b in bufs), msg

    for name in ("run_offsets", "heights", "widths", "group_offsets", "members", "out_run_offsets", "out_counts"):
        refused(INVALID, "null", nulls=(name,))
    if not entry_host:
        refused(INVALID, "unknown memspace 7", memspace=7)
    refused(SHAPE, "unknown op 4", op=4)
    refused(SHAPE, "unknown op -1", op=-1)
    refused(SHAPE, "n -1 is negative", n=-1)
    refused(SHAPE, "n_groups -2 is negative", G=-2)
    for bad_side in (0, 32768):
        h2 = hs.copy(); h2[3] = bad_side
        refused(SHAPE, f"RLE 3 is {bad_side}x5: height and width must lie in 1..32767", hs=h2)
        w2 = ws.copy(); w2[1] = bad_side
        refused(SHAPE, f"RLE 1 is 7x{bad_side}", ws=w2)
    down = offs.copy(); down[2] = down[1] - 1
    refused(SHAPE, "run_offsets decrease at RLE 1", offs=down)
    refused(SHAPE, "group_offsets[0] is 1, not 0", goffs=i64([1, 2, 4, 7]))
    refused(SHAPE, "group_offsets decrease at group 1: 1 after 2", goffs=i64([0, 2, 1, 7]))
    refused(SHAPE, "group 1 is empty", goffs=i64([0, 2, 2, 7]))
    refused(SHAPE, "group 2 member 1 is RLE 4: outside 0..3", mem=i64([0, 2, 1, 3, 2, 4, 2]))
    refused(SHAPE, "group 1 member 0 is RLE -1: outside 0..3", mem=i64([0, 2, -1, 3, 2, 0, 2]))
    refused(SHAPE, "group 1 member 1 (RLE 2) is 20x30, the group's first member (RLE 1) 7x5", mem=i64([0, 2, 1, 2, 2, 0, 2]))
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1, and RLE 3 (which no group need name) as well: the lowest is named
    bad[int(offs[3])] -= 1
    if entry_host:                                               # (the device entry finds a wrong total on the device: tests/test_gpu_rle_combine.py)
        for op in CC.OPS.values():
            refused(SHAPE, "RLE 1 sums to 38 pixels, its 7x5 plane has 35", counts=bad, op=op)
        unreferenced = counts.copy(); unreferenced[int(offs[3])] += 2
        refused(SHAPE, "RLE 3 sums to 37 pixels, its 7x5 plane has 35", counts=unreferenced, goffs=i64([0, 2]), mem=i64([0, 2]), G=1)


def test_size_query_small_capacity_and_no_groups():
    planes, counts, offs, hs, ws = _three()
    goffs, mem = CC.flat_groups(GROUPS)
    st, msg, want, want_offs, want_areas, want_boxes = CC.combine_host(counts, offs, hs, ws, goffs, mem, CC.XOR)
    assert st == 0, msg
    need = int(want_offs[3])
    assert want_areas.tolist() == [int((planes[0] ^ planes[2]).sum()), int((planes[1] ^ planes[3]).sum()), int(planes[0].sum())]
    lib = _mod("_lib")
    L = lib.lib()
    p = lambda a: a.ctypes.data
    o, a, b = np.full(4, 77, np.int64), np.full(3, 77, np.uint32), np.full((3, 4), 77, np.int32)
    head = (p(counts), p(offs), 4, p(hs), p(ws), p(goffs), p(mem), 3, CC.XOR)
    assert L.mrcnn_rle_combine_host(*head, None, 0, p(o), p(a), p(b)) == SHAPE      # the size query: capacity 0, out_counts NULL
    msg = L.mrcnn_last_error().decode()
    assert msg.startswith("rle_combine_host:") and f"capacity >= {need}" in msg
    assert o.tolist() == want_offs.tolist() and a.tolist() == want_areas.tolist() and (b == want_boxes).all()
    out = np.full(need + 5, 77, np.uint32)
    assert L.mrcnn_rle_combine_host(*head, p(out), need - 1, p(o), None, None) == SHAPE and (out == 77).all()
    assert f"holds {need - 1}: call again with capacity >= {need}" in L.mrcnn_last_error().decode()
    assert L.mrcnn_rle_combine_host(*head, p(out), need + 5, p(o), None, None) == 0
    assert out[:need].tolist() == want.tolist() and (out[need:] == 77).all()
    one = np.full(1, 77, np.int64)
    zero = np.zeros(1, np.int64)
    assert L.mrcnn_rle_combine_host(p(counts), p(offs), 4, p(hs), p(ws), p(zero), None, 0, CC.OR, None, 0, p(one), None, None) == 0    # n_groups = 0
    assert one.tolist() == [0]
    one[:] = 77
    assert L.mrcnn_rle_combine_host(None, p(zero), 0, None, None, p(zero), None, 0, CC.AND, None, 0, p(one), None, None) == 0          # n = 0
    assert one.tolist() == [0]


def test_a_result_past_the_first_guess_takes_the_wrappers_second_attempt(monkeypatch):
    """one 4 x 4 checkerboard of 13 runs, four groups of it alone: the wrapper guesses 13 + 2 * 4 + 2 = 23 runs, the result holds 52"""
    D, L = _mod("detection"), _mod("_lib").lib()
    yy, xx = np.mgrid[0:4, 0:4]
    runs = CC.encode(((xx + yy) % 2).astype(np.uint8))
    assert len(runs) == 13
    entry, capacities = L.mrcnn_rle_combine_host, []
    monkeypatch.setattr(L, "mrcnn_rle_combine_host", lambda *a: capacities.append(a[10]) or entry(*a))
    (counts, offs), areas, boxes = D.rle_combine_host((runs, np.array([0, 13], np.int64)), [(4, 4)], [[0], [0], [0], [0]], "or")
    assert capacities == [23, 52]
    assert counts.tolist() == runs.tolist() * 4 and offs.tolist() == [0, 13, 26, 39, 52]
    assert areas.tolist() == [8] * 4 and boxes.tolist() == [[0, 0, 4, 4]] * 4


# ---- 3. the helpers ------------------------------------------------------------------------------------------------------------------------
def disjoint_batch():
    """three images of different sizes, 7 rows each: overlapping ellipses, and rows that are not drawn — a score of 0, a score below
    min_score, an empty pixel box — with masks that would show if they were -> (det_src, rows, sizes, min_score, undrawn rows)"""
    from morph_cases import ellipse
    rng = np.random.default_rng(41)
    sizes = [(60, 80), (97, 45), (33, 65)]
    det = np.zeros((3, 7, 6), np.float32)
    rows = []
    for b, (h, w) in enumerate(sizes):
        row = []
        for i in range(7):
            cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
            p = ellipse(h, w, cy, cx, rng.uniform(0.1, 0.4) * h, rng.uniform(0.1, 0.4) * w)
            row.append({"size": [h, w], "counts": CC.encode(p)})
            det[b, i] = [0.1, 0.1, 0.9, 0.9, 1 + i % 3, 0.9 - 0.1 * i]
        rows.append(row)
    det[0, 2, 5] = 0.0                                           # not drawn: no score
    det[1, 0, 5] = 0.25                                          # not drawn: below min_score
    det[2, 3, :4] = [0.5, 0.5, 0.2, 0.9]                         # not drawn: an empty pixel box
    det[2, 6, 5] = np.nan
    return det, rows, sizes, 0.25, [(0, 2), (1, 0), (2, 3), (2, 6)]


def test_rle_disjoint_host_is_the_instance_map():
    D = _mod("detection")
    det, rows, sizes, min_score, undrawn = disjoint_batch()
    maps, visible = D.instance_map_rle_host(det, rows, sizes, min_score)
    got, areas, boxes = D.rle_disjoint_host(det, rows, sizes, min_score)
    assert areas.shape == (3, 7) and boxes.shape == (3, 7, 4) and (areas == visible).all()
    drawn = D.drawn_rows(det, sizes, min_score)
    assert sorted(zip(*np.nonzero(~drawn))) == undrawn
    overlaps = 0
    for b, (h, w) in enumerate(sizes):
        for i in range(7):
            plane = CC.decode(got[b][i]["counts"], h, w)
            assert got[b][i]["size"] == [h, w] and (plane == (maps[b] == i)).all(), (b, i)
            own = CC.decode(rows[b][i]["counts"], h, w)
            assert own.any()
            overlaps += drawn[b, i] and plane.sum() < own.sum()
            if (b, i) in undrawn:
                assert got[b][i]["counts"].tolist() == [h * w]
    assert overlaps > 5
    pair = (np.concatenate([e["counts"] for r in rows for e in r]), np.concatenate(([0], np.cumsum([len(e["counts"]) for r in rows for e in r]))).astype(np.int64))
    (c, o), a2, _ = D.rle_disjoint_host(det, pair, sizes, min_score)                 # a pair in, a pair out
    assert c.tolist() == np.concatenate([e["counts"] for r in got for e in r]).tolist() and len(o) == 22 and a2.tolist() == areas.reshape(-1).tolist()


def test_pairwise_helpers_and_groups():
    D = _mod("detection")
    _det, rows, sizes, _, _ = disjoint_batch()
    A = [r[:3] for r in rows]
    B = [r[3:6] for r in rows]
    for f, rule in ((D.rle_union_host, np.bitwise_or), (D.rle_intersection_host, np.bitwise_and), (D.rle_xor_host, np.bitwise_xor),
                    (D.rle_difference_host, lambda a, b: a & (1 - b))):
        got = f(A, other=B)
        for b, (h, w) in enumerate(sizes):
            for i in range(3):
                want = rule(CC.decode(A[b][i]["counts"], h, w), CC.decode(B[b][i]["counts"], h, w))
                assert got[b][i]["size"] == [h, w] and got[b][i]["counts"].tolist() == CC.encode(want).tolist()
    as_lists = D.rle_union_host(rows, groups=[[0, 1, 2], [20, 14]])
    as_pair = D.rle_union_host(rows, groups=(np.array([0, 3, 5]), np.array([0, 1, 2, 20, 14])))
    assert [r["counts"].tolist() for r in as_lists] == [r["counts"].tolist() for r in as_pair] and [r["size"] for r in as_lists] == [[60, 80], [33, 65]]
    with pytest.raises(ValueError):
        D.rle_union_host(rows)
    with pytest.raises(ValueError):
        D.rle_combine_host(rows, None, [[0, 1]], "nand")
    with pytest.raises(RuntimeError, match="group 0 member 1"):
        D.rle_union_host(rows, groups=[[0, 7]])                  # two sizes in one group: the library's text


def test_the_union_of_the_split_parts_is_the_mask():
    D = _mod("detection")
    rng = np.random.default_rng(43)
    planes = [(rng.random((40, 30)) < 0.3).astype(np.uint8), np.zeros((40, 30), np.uint8), (rng.random((17, 90)) < 0.6).astype(np.uint8)]
    rows = [[{"size": [40, 30], "counts": CC.with_zero_runs(CC.encode(planes[0]), rng)}, {"size": [40, 30], "counts": CC.encode(planes[1])}],
            [{"size": [17, 90], "counts": CC.encode(planes[2])}, {"size": [17, 90], "counts": CC.encode(planes[2])}]]
    parts, parent = D.rle_split_components_host(rows, None)
    assert len(parts) > 20
    keep = [k for k in range(4) if (parent == k).any()]          # a mask without a component has no part: a group needs a member
    assert keep == [0, 2, 3]
    pair = CC.flat_set([p["counts"] for p in parts])
    united, areas, _ = D.rle_combine_host(pair, [tuple(p["size"]) for p in parts], [np.flatnonzero(parent == k).tolist() for k in keep], "or")
    for g, k in enumerate(keep):
        got = united[0][int(united[1][g]):int(united[1][g + 1])]
        assert got.tolist() == CC.encode(planes[[0, 1, 2, 2][k]]).tolist() and int(areas[g]) == int(planes[[0, 1, 2, 2][k]].sum())


# ---- 4. C over the header ------------------------------------------------------------------------------------------------------------------
C_PROGRAM = r"""
#include <stdio.h>
#include "maskrcnn_hip.h"
int main(void)
{
    /* two 3x2 planes: columns [1 1 0 | 0 0 0] and [0 1 1 | 1 0 0] */
    const uint32_t counts[] = {0, 2, 4, 1, 3, 2};
    const int64_t run_offsets[] = {0, 3, 6};
    const int32_t hs[] = {3, 3}, ws[] = {2, 2};
    const int64_t group_offsets[] = {0, 2, 4}, members[] = {0, 1, 1, 0}, empty_group[] = {0, 2, 2};
    uint32_t out[16], areas[2];
    int64_t offs[3];
    int32_t boxes[8];
    int op, st;
    for (op = MRCNN_RLE_OR; op <= MRCNN_RLE_DIFF; ++op) {
        int64_t j;
        st = mrcnn_rle_combine_host(counts, run_offsets, 2, hs, ws, group_offsets, members, 2, op, out, 16, offs, areas, boxes);
        if (st != MRCNN_OK) { fprintf(stderr, "%s\n", mrcnn_last_error()); return st; }
        printf("op %d areas %u %u runs", op, (unsigned)areas[0], (unsigned)areas[1]);
        for (j = 0; j < offs[2]; ++j) printf(" %u", (unsigned)out[j]);
        printf("\n");
    }
    /* the device entry answers an argument error before it looks for a device */
    st = mrcnn_rle_combine(counts, run_offsets, 2, hs, ws, empty_group, members, 2, MRCNN_RLE_OR, MRCNN_HOST, out, 16, offs, NULL, NULL);
    printf("status %d: %s\n", st, mrcnn_last_error());
    st = mrcnn_rle_combine(counts, run_offsets, 2, hs, ws, group_offsets, members, 2, 9, MRCNN_HOST, NULL, 0, offs, NULL, NULL);
    printf("status %d: %s\n", st, mrcnn_last_error());
    return 0;
}
"""


def test_a_c_program_calls_both_entries(pkg, tmp_path):
    libdir = os.path.dirname(_mod("_lib").SO_PATH)
    src = tmp_path / "combine.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "combine")
    for std in ("-std=c99", "-std=c11"):
        r = subprocess.run(["gcc", std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                            "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    a = np.array([[1, 0], [1, 0], [0, 0]], np.uint8)
    b = np.array([[0, 1], [1, 0], [1, 0]], np.uint8)
    for op, line in zip(range(4), lines):
        first, second = CC.reference([a, b], op), CC.reference([b, a], op)
        runs = CC.encode(first).tolist() + CC.encode(second).tolist()
        assert line == f"op {op} areas {int(first.sum())} {int(second.sum())} runs " + " ".join(str(v) for v in runs), (line, runs)
    assert lines[4].startswith("status 4: rle_combine: group 1 is empty") and lines[5].startswith("status 4: rle_combine: unknown op 9")


def test_the_example_makes_the_masks_disjoint_before_it_traces(pkg, tmp_path):
    """examples/maskrcnn_polygons.c --disjoint, run with --host: the rings are those of every mask minus the masks before it"""
    from morph_cases import ellipse
    from test_c_host_components import _write_set
    D = _mod("detection")
    libdir = os.path.dirname(_mod("_lib").SO_PATH)
    src = os.path.join(ROOT, "examples", "maskrcnn_polygons.c")
    text = open(src).read()
    assert "mrcnn_rle_combine(" in text and "mrcnn_rle_combine_host(" in text and "--disjoint" in text
    exe = str(tmp_path / "maskrcnn_polygons")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, src, "-L", libdir, "-lmaskrcnn_hip", f"-Wl,-rpath,{libdir}",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--disjoint"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 64 and "[--disjoint] <set.txt>" in r.stderr
    planes = [[ellipse(40, 50, 20, 20, 12, 15), ellipse(40, 50, 20, 30, 12, 15), ellipse(40, 50, 25, 25, 14, 20)],
              [np.ones((30, 20), np.uint8), ellipse(30, 20, 15, 10, 5, 5), np.zeros((30, 20), np.uint8)]]
    sizes = [(40, 50), (30, 20)]
    f = tmp_path / "set.txt"
    _write_set(f, planes)
    rows = [[{"size": list(p.shape), "counts": CC.encode(p)} for p in row] for row in planes]

    def lines_of(rles):
        rings, areas = D.rle_to_polygons_host(rles, sizes)
        return [f"RLE {3 * b + i} ring {k} area {int(area)}: " + " ".join(f"{int(x)},{int(y)}" for x, y in ring)
                for b in range(2) for i in range(3) for k, (ring, area) in enumerate(zip(rings[b][i], areas[b][i]))]

    def run(*flags):
        r = subprocess.run([exe, "--host", *flags, str(f)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return [line.strip() for line in r.stdout.strip().splitlines()[1:]]

    det = np.tile(np.array([0.0, 0.0, 1.0, 1.0, 1.0, 0.9], np.float32), (2, 3, 1))           # every row drawn
    want, areas, _ = D.rle_disjoint_host(det, rows, sizes)
    assert areas[1].tolist() == [600, 0, 0] and 0 < areas[0, 2] < planes[0][2].sum()
    assert run() == lines_of(rows) and run("--disjoint") == lines_of(want) != lines_of(rows)
    assert run("--disjoint", "--min-area", "3") == run("--min-area", "3", "--disjoint") == lines_of(D.rle_disjoint_host(det, D.rle_remove_small_host(rows, sizes, 3), sizes)[0])
    bad = tmp_path / "bad.txt"
    bad.write_text("1 1\n4 5 2 3 3\n")                          # sums to 6, the plane has 20: the library's text, the status as exit code
    r = subprocess.run([exe, "--host", "--disjoint", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "rle_combine_host: RLE 0 sums to 6 pixels" in r.stderr, r.stderr
