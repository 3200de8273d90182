"""The set algebra of run-length masks on the GPU (mrcnn_rle_combine; detection.rle_combine, rle_disjoint and the pairwise helpers;
predict_tiled(disjoint=True)).  Every comparison is bit for bit against the sequential host definition, which
tests/test_rle_combine_host.py pins against a numpy restatement on dense planes: out_counts, out_run_offsets, areas and bboxes_xywh,
from host memory and from device tensors.

The cases (tests/combine_cases.py) cross the word rows of the packed bit box (sides 31..33, 63..65), put several blocks and several
plane sizes into one call, wrap runs over column ends, fold a group of 100 members with duplicates in one thread's loop, and pass the
1024 rows a thread folds per pass (the 1100x9 plane)."""
import importlib

import numpy as np
import pytest

import combine_cases as CC
import morph_cases as MC
import unite_cases as UC
from test_gpu_rle_morph import _cuda, _iou_with_itself, _synthetic_batch

pytestmark = pytest.mark.gpu
SHAPE = CC.SHAPE


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _flat(host_definition, device, counts, offs, hs, ws, goffs, mem, op):
    D, M = _mod("detection"), _mod("_marshal")
    return D._combine_flat(host_definition, M.Space(device), counts, offs, np.ascontiguousarray(hs, np.int32), np.ascontiguousarray(ws, np.int32),
                           np.ascontiguousarray(goffs, np.int64), np.ascontiguousarray(mem, np.int64), op)


def _both_memspaces_equal_the_definition(runs, hs, ws, groups, op, what):
    """the device entry from host memory and from device tensors against the host entry -> the host's four arrays"""
    counts, offs = CC.flat_set(runs)
    goffs, mem = CC.flat_groups(groups)
    want = _flat(True, None, counts, offs, hs, ws, goffs, mem, op)
    got = _flat(False, None, counts, offs, hs, ws, goffs, mem, op)
    assert isinstance(got[0], np.ndarray), what
    MC.assert_same(got, want, f"{what}, host memory")
    dev = _flat(False, "cuda", _cuda(counts), _cuda(offs), hs, ws, goffs, mem, op)
    assert all(a.is_cuda for a in dev), what
    MC.assert_same(dev, want, f"{what}, device memory")
    return want


@pytest.fixture(scope="module")
def cases(pkg):
    return CC.all_cases()


# ---- 1. device against host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(CC.OPS))
def test_one_ragged_call_over_all_the_groups(cases, op):
    assert len(cases["groups"]) > 200
    want = _both_memspaces_equal_the_definition(cases["runs"], cases["hs"], cases["ws"], cases["groups"], CC.OPS[op], f"all groups, {op}")
    assert (want[2] == 0).any() and (want[2] > 0).any()


@pytest.mark.parametrize("name", ["g100/33x65", "g17/1100x9", "rand0+rand1/1100x9", "full+rand0/1100x9", "comb+checkerboard/130x40", "comb/65x33",
                                  "rand0+rand1/1x1", "full/1x1", "all_empty/64x32", "rand0+rand0/63x31", "ellipse_a+ellipse_c/32x64"])
def test_single_groups(cases, name):
    runs, hs, ws, groups, planes = CC.only(cases, name)
    for op in CC.OPS.values():
        want = _both_memspaces_equal_the_definition(runs, hs, ws, groups, op, f"{name}, op {op}")
        assert want[0].view(np.uint32).tolist() == CC.encode(CC.reference([planes[k] for k in groups[0]], op)).tolist()


def test_a_result_past_the_first_guess_takes_the_wrappers_second_attempt(pkg, monkeypatch):
    """one 4 x 4 checkerboard of 13 runs, four groups of it alone: the wrapper guesses 13 + 2 * 4 + 2 = 23 runs, the result holds 52"""
    L = _mod("_lib").lib()
    yy, xx = np.mgrid[0:4, 0:4]
    runs = CC.encode(((xx + yy) % 2).astype(np.uint8))
    entry, capacities = L.mrcnn_rle_combine, []
    monkeypatch.setattr(L, "mrcnn_rle_combine", lambda *a: capacities.append(a[11]) or entry(*a))
    want = _both_memspaces_equal_the_definition([runs], [4], [4], [[0], [0], [0], [0]], CC.OR, "four copies of a checkerboard")
    assert capacities == [23, 52, 23, 52]                        # from host memory, then from device tensors
    assert want[0].tolist() == runs.tolist() * 4 and want[1].tolist() == [0, 13, 26, 39, 52] and want[2].tolist() == [8] * 4


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------------------
def _device_call(counts, offs, hs, ws, groups, op, capacity, fill=77, out=True):
    """mrcnn_rle_combine on device tensors with pre-filled outputs -> (status, message, [out_counts, out_run_offsets, areas, bboxes])"""
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n, G = len(offs) - 1, len(groups)
    goffs, mem = CC.flat_groups(groups)
    c_g, o_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64))
    hs, ws = (np.ascontiguousarray(a, np.int32) for a in (hs, ws))
    bufs = [torch.full((max(1, capacity),), fill, dtype=torch.int32, device="cuda"), torch.full((G + 1,), fill, dtype=torch.int64, device="cuda"),
            torch.full((max(1, G),), fill, dtype=torch.int32, device="cuda"), torch.full((max(1, G), 4), fill, dtype=torch.int32, device="cuda")]
    st = L.mrcnn_rle_combine(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, goffs.ctypes.data, mem.ctypes.data, G, op, lib.DEVICE,
                             bufs[0].data_ptr() if out else None, capacity if out else 0, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr())
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs]


def _four():
    planes = [MC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), MC.ellipse(20, 30, 12, 12, 5, 5), MC.ellipse(7, 5, 3, 2, 2, 1)]
    runs = [CC.encode(p) for p in planes]
    return planes, *CC.flat_set(runs), [20, 7, 20, 7], [30, 5, 30, 5]


GROUPS = [[0, 2], [1, 3], [2, 0, 2]]


def test_a_bad_total_on_the_device_is_named_and_nothing_is_written(pkg):
    _planes, counts, offs, hs, ws = _four()
    st, msg, bufs = _device_call(counts, offs, hs, ws, GROUPS, CC.OR, 128)
    assert st == 0 and bufs[1][0] == 0, msg
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1, and RLE 3 as well: the lowest is named
    bad[int(offs[3])] -= 1
    for op in CC.OPS.values():
        st, msg, bufs = _device_call(bad, offs, hs, ws, GROUPS, op, 128)
        assert st == SHAPE and msg.startswith("rle_combine:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg, msg
        assert all((b == 77).all() for b in bufs)
    unreferenced = counts.copy()
    unreferenced[int(offs[3])] += 2                              # an RLE no group names is judged too
    st, msg, bufs = _device_call(unreferenced, offs, hs, ws, [[0, 2]], CC.AND, 128)
    assert st == SHAPE and "RLE 3 sums to 37 pixels, its 7x5 plane has 35" in msg and all((b == 77).all() for b in bufs)
    down = offs.copy()
    down[2] = down[1] - 1
    st, msg, bufs = _device_call(counts, down, hs, ws, GROUPS, CC.OR, 128)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg and all((b == 77).all() for b in bufs)


def test_the_size_query_and_a_small_capacity_on_the_device(pkg):
    _planes, counts, offs, hs, ws = _four()
    want = _flat(True, None, counts, offs, hs, ws, *CC.flat_groups(GROUPS), CC.XOR)
    need = int(want[1][3])
    st, msg, bufs = _device_call(counts, offs, hs, ws, GROUPS, CC.XOR, 0, out=False)                            # capacity 0, out_counts NULL
    assert st == SHAPE and f"capacity >= {need}" in msg and msg.startswith("rle_combine:")
    assert bufs[1].tolist() == want[1].tolist() and bufs[2].view(np.uint32).tolist() == want[2].tolist() and (bufs[3] == want[3]).all()
    st, msg, bufs = _device_call(counts, offs, hs, ws, GROUPS, CC.XOR, need - 1)
    assert st == SHAPE and f"capacity >= {need}" in msg and (bufs[0] == 77).all() and bufs[1].tolist() == want[1].tolist()
    st, msg, bufs = _device_call(counts, offs, hs, ws, GROUPS, CC.XOR, need + 5)
    assert st == 0 and bufs[0][:need].view(np.uint32).tolist() == want[0].tolist() and (bufs[0][need:] == 77).all()
    st, msg, bufs = _device_call(counts, offs, hs, ws, [], CC.OR, 8)                                            # n_groups = 0
    assert st == 0 and bufs[1].tolist() == [0] and (bufs[0] == 77).all(), msg
    import torch
    lib = _mod("_lib")
    o = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    zero = np.zeros(1, np.int64)
    assert lib.lib().mrcnn_rle_combine(None, z.data_ptr(), 0, None, None, zero.ctypes.data, None, 0, CC.DIFF, lib.DEVICE, None, 0, o.data_ptr(), None, None) == 0   # n = 0
    assert o.cpu().tolist() == [0]


# ---- 3. resident flows -------------------------------------------------------------------------------------------------------------------
def _resident_flow(pair_g, det_src_g, sizes, slots):
    """a resident (counts, run_offsets) pair made disjoint where it lies and handed on to the polygon and IoU entries, against the host
    route from the same runs and against the instance map"""
    D, lib = _mod("detection"), _mod("_lib")
    n = len(sizes) * slots
    pair_h = (pair_g[0].cpu().numpy().view(np.uint32), pair_g[1].cpu().numpy())
    det_h = det_src_g.cpu().numpy()
    got, areas, boxes = D.rle_disjoint(det_src_g, pair_g, sizes)
    assert got[0].is_cuda and got[1].is_cuda and areas.is_cuda and boxes.is_cuda
    want, w_areas, w_boxes = D.rle_disjoint_host(det_h, pair_h, sizes)
    MC.assert_same((got[0], got[1], areas, boxes), (want[0], want[1], w_areas, w_boxes), "resident, disjoint")
    maps, visible = D.instance_map_rle(det_src_g, pair_g, sizes, 0.0)
    assert (areas.cpu().numpy().view(np.uint32).reshape(len(sizes), slots) == visible.cpu().numpy().view(np.uint32)).all()
    planes = D.rle_decode_planes(got, sizes)
    for b in range(len(sizes)):
        ids = np.arange(slots).reshape(slots, 1, 1)
        assert planes[b].is_cuda and (planes[b].cpu().numpy() == (maps[b].cpu().numpy()[None] == ids)).all(), b
    before = sum(int(pair_h[0][int(pair_h[1][k]):int(pair_h[1][k + 1])][1::2].sum()) for k in range(n))
    assert 0 < int(w_areas.sum()) <= before
    rings =D.rle_to_polygons(got, sizes, flat=True)
    assert rings["xy"].is_cuda
    rings_h = D.rle_to_polygons_host(want, sizes, flat=True)
    for key in ("rle_rings", "ring_offsets", "ring_areas", "xy"):
        assert (rings[key].cpu().numpy() == rings_h[key]).all(), key
    iou = _iou_with_itself(lib, got, got, n, slots, lib.DEVICE)
    iou_h = _iou_with_itself(lib, want, want, n, slots, lib.HOST)
    assert iou.tobytes() == iou_h.tobytes()
    iou = iou.reshape(len(sizes), slots, slots)
    off_diagonal = ~np.eye(slots, dtype=bool)
    assert (iou[:, off_diagonal] == 0.0).all() and (iou[:, ~off_diagonal] == 1.0).any()    # two different rows of an image share no pixel
    # the pairwise helpers on the resident pair: every row clipped to its image's first row, and what the clip left out
    first = np.repeat(np.arange(len(sizes)) * slots, slots)
    groups = [[k, int(first[k])] for k in range(n)]
    for op in ("and", "diff", "xor", "or"):
        g, a, bx = D.rle_combine(pair_g, sizes, groups, op)
        w, wa, wb = D.rle_combine_host(pair_h, sizes, groups, op)
        assert g[0].is_cuda and a.is_cuda
        MC.assert_same((g[0], g[1], a, bx), (w[0], w[1], wa, wb), f"resident, {op}")
    clipped = D.rle_intersection(pair_g, sizes, other=pair_g)
    assert clipped[0].is_cuda and (clipped[1].cpu().numpy() == D.rle_intersection_host(pair_h, sizes, other=pair_h)[1]).all()
    return int(w_areas.sum()), before


def test_the_runs_of_masks_rle_source_are_made_disjoint_where_they_lie(pkg):
    import torch
    CE = _mod("coco_eval")
    det, masks, sizes, H, W = _synthetic_batch()
    batch = CE.device_detections([1, 2, 3], torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, H, W, 0.5)
    n = len(sizes) * batch.rows
    D = _mod("detection")
    det_src = D.masks_rle_source(torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, H, W, 0.5)[0]
    after, before = _resident_flow((batch.counts, batch.run_offsets[:n + 1]), det_src, sizes, batch.rows)
    assert after < before                                        # ten random masks per image: some of them overlapped


def test_the_runs_of_unite_tiles_are_made_disjoint_where_they_lie(pkg):
    import tiles_cases as TC
    D = _mod("detection")
    sc = next(s for s in UC.scenes() if s["name"] == "two_images")
    resident = []
    out = D._merge_tiles(False, _cuda(sc["det"]), _cuda(sc["masks"]), sc["tiles"], sc["sizes"], TC.MODEL, TC.MODEL, 0.5, "iou", 0.5, sc["max_out"], unite=True,
                         resident=resident)
    sizes = [tuple(s) for s in sc["sizes"]]
    _resident_flow(resident[0], out[0], sizes, int(sc["max_out"]))


# ---- 4. predict_tiled(disjoint=) -----------------------------------------------------------------------------------------------------------
def test_predict_tiled_makes_the_kept_masks_disjoint(pkg, small_model):
    d, _cfg = small_model
    D = _mod("detection")
    m = _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")
    rng = np.random.default_rng(21)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(200, 333), (300, 260)]]
    sizes = [(200, 333), (300, 260)]
    kw = dict(overlap=(32, 48), metric="iou", max_out=6, unite=True, link_threshold=0.25, polygons=True)
    plain = m.predict_tiled(images, **kw)
    disjoint = m.predict_tiled(images, disjoint=True, **kw)
    want, areas, _ = D.rle_disjoint_host(np.asarray(plain[0]), plain[3], sizes)
    assert int(areas.sum()) > 0
    for b in range(2):
        for i in range(6):
            assert disjoint[3][b][i]["size"] == want[b][i]["size"] and disjoint[3][b][i]["counts"].tolist() == want[b][i]["counts"].tolist(), (b, i)
    for k in range(3):
        assert (np.asarray(disjoint[k]) == np.asarray(plain[k])).all()
    rings_h, _areas_h = D.rle_to_polygons_host(want, sizes)
    for b in range(2):
        for i in range(6):
            assert len(disjoint[4][0][b][i]) == len(rings_h[b][i]) and all((p == q).all() for p, q in zip(disjoint[4][0][b][i], rings_h[b][i]))
