"""Moving run-length masks to another pixel grid on the GPU (mrcnn_rle_transform; detection.rle_transform, rle_crop, rle_place, rle_flip,
rle_rot90, rle_resize).  Every comparison is bit for bit against the sequential host definition, which
tests/test_rle_transform_host.py pins against a numpy restatement on dense planes: out_counts, out_run_offsets, areas and bboxes_xywh,
from host memory and from device tensors.  The host definition evaluates the forward rule pixel by pixel; the kernel works from the
closed-form inverse: device against host is closed form against brute force.

The cases (tests/transform_cases.py) cross the word rows of the packed bit box (sides 31..33, 63..65), put several blocks, several
plane sizes and both kinds of record into one call, wrap runs over column ends, give negative numerators (overhanging windows, flips),
empty work boxes (a window wholly outside), and pass the 1024 rows a thread fills per pass before and after a transposition (1100x9,
9x1100, and the 3x enlargement of 1100 rows)."""
import importlib

import numpy as np
import pytest

import combine_cases as CC
import morph_cases as MC
import transform_cases as TC
from test_gpu_rle_morph import _cuda, _synthetic_batch

pytestmark = pytest.mark.gpu
SHAPE = TC.SHAPE


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _flat(host_definition, device, counts, offs, hs, ws, ohs, ows, xf):
    D, M = _mod("detection"), _mod("_marshal")
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return D._transform_flat(host_definition, M.Space(device), counts, offs, i32(hs), i32(ws), i32(ohs), i32(ows), np.ascontiguousarray(xf, np.int64))


def _both_memspaces_equal_the_definition(runs, hs, ws, ohs, ows, xf, what):
    """the device entry from host memory and from device tensors against the host entry -> the host's four arrays"""
    counts, offs = TC.flat_set(runs)
    want = _flat(True, None, counts, offs, hs, ws, ohs, ows, xf)
    got = _flat(False, None, counts, offs, hs, ws, ohs, ows, xf)
    assert isinstance(got[0], np.ndarray), what
    MC.assert_same(got, want, f"{what}, host memory")
    dev = _flat(False, "cuda", _cuda(counts), _cuda(offs), hs, ws, ohs, ows, xf)
    assert all(a.is_cuda for a in dev), what
    MC.assert_same(dev, want, f"{what}, device memory")
    return want


@pytest.fixture(scope="module")
def cases(pkg):
    return TC.all_cases()


# ---- 1. device against host --------------------------------------------------------------------------------------------------------------
def test_one_ragged_call_over_all_the_cases(cases):
    n = len(cases["names"])
    flags = cases["xf"][:, 0]
    assert n > 200 and (flags == 1).sum() > 100 and (flags == 0).sum() > 100
    want = _both_memspaces_equal_the_definition(cases["runs"], cases["hs"], cases["ws"], cases["ohs"], cases["ows"], cases["xf"], "all cases")
    assert (want[2] == 0).any() and (want[2] > 0).any()


def _pool_mask(h, w, name):
    return CC.pool(h, w, np.random.default_rng(h * 1000 + w))[CC.POOL.index(name)]


def _singles():
    """{name: (plane, record, (oh, ow))}"""
    rng = np.random.default_rng(3)
    out = {}
    for rname, r, osz in TC.records_of(1, 1, rng):
        if not rname.startswith("random"):
            out[f"1x1/{rname}"] = (np.ones((1, 1), np.uint8), r, osz)
    comb = _pool_mask(65, 33, "comb")
    for t in (0, 1):
        for fx in (0, 1):
            for fy in (0, 1):
                out[f"comb/65x33/sym_t{t}x{fx}y{fy}"] = (comb, *TC.symmetry(65, 33, t, fx, fy))
    for h, w in ((1100, 9), (9, 1100)):
        for fx, fy in ((0, 0), (1, 1), (0, 1)):
            out[f"rand0/{h}x{w}/sym_t1x{fx}y{fy}"] = (_pool_mask(h, w, "rand0"), *TC.symmetry(h, w, 1, fx, fy))
        out[f"rand0/{h}x{w}/resize_transpose"] = (_pool_mask(h, w, "rand0"), *[x for x in TC.records_of(h, w, rng) if x[0] == "resize_transpose"][0][1:])
    r63 = _pool_mask(63, 31, "rand0")
    for p, q in ((3, 2), (2, 3)):
        for rule in ("center", "floor"):
            out[f"rand0/63x31/resize_{p}/{q}_{rule}"] = (r63, *TC.resize(63, 31, TC.scaled(63, p, q), TC.scaled(31, p, q), rule))
    e = _pool_mask(33, 65, "ellipse_a")
    out["ellipse_a/33x65/crop_outside"] = (e, *TC.crop(67, -1, 5, 34))
    out["ellipse_a/33x65/crop_all_sides"] = (e, *TC.crop(-3, -3, 71, 39))
    out["full/33x65/crop_all_sides"] = (np.ones((33, 65), np.uint8), *TC.crop(-3, -3, 71, 39))
    return out


SINGLES = _singles()


@pytest.mark.parametrize("name", sorted(SINGLES))
def test_single_cases(pkg, name):
    plane, r, (oh, ow) = SINGLES[name]
    h, w = plane.shape
    want = _both_memspaces_equal_the_definition([TC.encode(plane)], [h], [w], [oh], [ow], r[None], name)
    ref = TC.reference(plane, r, oh, ow)
    assert want[0].view(np.uint32).tolist() == TC.encode(ref).tolist() and (int(want[2][0]), want[3][0].tolist()) == TC.stats(ref)
    if name.endswith("crop_outside"):
        assert want[0].tolist() == [oh * ow]
    if name == "1x1/1x1_to_65x33":
        assert want[0].tolist() == [0, 65 * 33]


def test_the_single_cases_are_what_their_names_say():
    assert {"1x1/identity", "1x1/1x1_to_65x33", "comb/65x33/sym_t1x1y0", "rand0/1100x9/sym_t1x0y0", "rand0/9x1100/sym_t1x1y1", "rand0/63x31/resize_3/2_floor",
            "rand0/63x31/resize_2/3_center", "ellipse_a/33x65/crop_outside", "ellipse_a/33x65/crop_all_sides"} <= set(SINGLES)
    assert sum(k.startswith("comb/65x33/sym_") for k in SINGLES) == 8


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------------------
def _device_call(counts, offs, hs, ws, ohs, ows, xf, capacity, fill=77, out=True):
    """mrcnn_rle_transform on device tensors with pre-filled outputs -> (status, message, [out_counts, out_run_offsets, areas, bboxes])"""
    import torch
    lib = _mod("_lib")
    L = lib.lib()
    n = len(offs) - 1
    c_g, o_g = _cuda(np.asarray(counts, np.uint32)), _cuda(np.asarray(offs, np.int64))
    hs, ws, ohs, ows = (np.ascontiguousarray(a, np.int32) for a in (hs, ws, ohs, ows))
    xf = np.ascontiguousarray(xf, np.int64)
    bufs = [torch.full((max(1, capacity),), fill, dtype=torch.int32, device="cuda"), torch.full((n + 1,), fill, dtype=torch.int64, device="cuda"),
            torch.full((max(1, n),), fill, dtype=torch.int32, device="cuda"), torch.full((max(1, n), 4), fill, dtype=torch.int32, device="cuda")]
    st = L.mrcnn_rle_transform(c_g.data_ptr(), o_g.data_ptr(), n, hs.ctypes.data, ws.ctypes.data, ohs.ctypes.data, ows.ctypes.data, xf.ctypes.data, lib.DEVICE,
                               bufs[0].data_ptr() if out else None, capacity if out else 0, bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr())
    torch.cuda.synchronize()
    return st, L.mrcnn_last_error().decode(), [b.cpu().numpy() for b in bufs]


def _four():
    planes = [MC.ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), MC.ellipse(20, 30, 12, 12, 5, 5), MC.ellipse(7, 5, 3, 2, 2, 1)]
    runs = [TC.encode(p) for p in planes]
    xf = np.stack([TC.symmetry(20, 30, 1, 0, 1)[0], TC.crop(-1, -1, 8, 9)[0], TC.resize(20, 30, 30, 45, "center")[0], TC.crop(9, 0, 2, 2)[0]])
    return planes, *TC.flat_set(runs), [20, 7, 20, 7], [30, 5, 30, 5], [30, 9, 30, 2], [20, 8, 45, 2], xf


def test_a_bad_total_on_the_device_is_named_and_nothing_is_written(pkg):
    _planes, counts, offs, hs, ws, ohs, ows, xf = _four()
    st, msg, bufs = _device_call(counts, offs, hs, ws, ohs, ows, xf, 256)
    assert st == 0 and bufs[1][0] == 0, msg
    bad = counts.copy()
    bad[int(offs[1]) + 1] += 3                                   # RLE 1, and RLE 3 as well: the lowest is named
    bad[int(offs[3])] -= 1
    st, msg, bufs = _device_call(bad, offs, hs, ws, ohs, ows, xf, 256)
    assert st == SHAPE and msg.startswith("rle_transform:") and "RLE 1 sums to 38 pixels, its 7x5 plane has 35" in msg, msg
    assert all((b == 77).all() for b in bufs)
    down = offs.copy()
    down[2] = down[1] - 1
    st, msg, bufs = _device_call(counts, down, hs, ws, ohs, ows, xf, 256)
    assert st == SHAPE and "run_offsets decrease at RLE 1" in msg and all((b == 77).all() for b in bufs)


def test_the_size_query_and_a_small_capacity_on_the_device(pkg):
    _planes, counts, offs, hs, ws, ohs, ows, xf = _four()
    want = _flat(True, None, counts, offs, hs, ws, ohs, ows, xf)
    need = int(want[1][4])
    st, msg, bufs = _device_call(counts, offs, hs, ws, ohs, ows, xf, 0, out=False)                              # capacity 0, out_counts NULL
    assert st == SHAPE and f"capacity >= {need}" in msg and msg.startswith("rle_transform:")
    assert bufs[1].tolist() == want[1].tolist() and bufs[2].view(np.uint32).tolist() == want[2].tolist() and (bufs[3] == want[3]).all()
    st, msg, bufs = _device_call(counts, offs, hs, ws, ohs, ows, xf, need - 1)
    assert st == SHAPE and f"capacity >= {need}" in msg and (bufs[0] == 77).all() and bufs[1].tolist() == want[1].tolist()
    st, msg, bufs = _device_call(counts, offs, hs, ws, ohs, ows, xf, need + 5)
    assert st == 0 and bufs[0][:need].view(np.uint32).tolist() == want[0].tolist() and (bufs[0][need:] == 77).all()
    import torch
    lib = _mod("_lib")
    o = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.lib().mrcnn_rle_transform(None, z.data_ptr(), 0, None, None, None, None, None, lib.DEVICE, None, 0, o.data_ptr(), None, None) == 0    # n = 0
    assert o.cpu().tolist() == [0]


# ---- 3. the resident flow ------------------------------------------------------------------------------------------------------------------
def test_the_runs_of_masks_rle_source_are_moved_where_they_lie(pkg):
    import torch
    CE, D = _mod("coco_eval"), _mod("detection")
    det, masks, sizes, H, W = _synthetic_batch()
    batch = CE.device_detections([1, 2, 3], torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, H, W, 0.5)
    slots = batch.rows
    n = len(sizes) * slots
    pair_g = (batch.counts, batch.run_offsets[:n + 1])
    pair_h = (pair_g[0].cpu().numpy().view(np.uint32), pair_g[1].cpu().numpy())
    windows = [(40, 30, 200, 150), (-10, 100, 300, 200), (50, 60, 150, 250)]                 # the second reaches outside its image

    def same(got, want, what):
        assert got[0][0].is_cuda and got[0][1].is_cuda and got[1].is_cuda and got[2].is_cuda, what
        MC.assert_same((got[0][0], got[0][1], got[1], got[2]), (want[0][0], want[0][1], want[1], want[2]), what)
        assert got[3] == want[3], what

    # a resident pair cropped where it lies
    crop_g = D.rle_crop(pair_g, sizes, windows)
    crop_h = D.rle_crop_host(pair_h, sizes, windows)
    same(crop_g, crop_h, "resident, crop")
    assert crop_g[3] == [(150, 200), (200, 300), (250, 150)] and int(crop_h[1].sum()) > 0

    # the crop put back into its frame is the original clipped to the window: rle_combine's intersection with the window's rectangle
    origins = [(x, y) for x, y, _, _ in windows]
    placed = D.rle_place(crop_g[0], crop_g[3], origins, sizes)
    same(placed, D.rle_place_host(crop_h[0], crop_h[3], origins, sizes), "resident, place")
    assert placed[3] == [tuple(s) for s in sizes]
    rects = []
    for (h, w), (x, y, ww, wh) in zip(sizes, windows):
        r = np.zeros((h, w), np.uint8)
        r[max(y, 0):y + wh, max(x, 0):x + ww] = 1
        rects += [TC.encode(r)] * slots
    rect_pair = TC.flat_set(rects)
    clipped = D.rle_intersection(pair_g, sizes, other=(_cuda(rect_pair[0]), _cuda(rect_pair[1])))
    assert clipped[0].is_cuda
    assert (clipped[1].cpu().numpy() == placed[0][1].cpu().numpy()).all() and (clipped[0].cpu().numpy() == placed[0][0].cpu().numpy()).all()
    before = np.array([int(pair_h[0][int(pair_h[1][k]):int(pair_h[1][k + 1])][1::2].sum()) for k in range(n)])
    after = placed[1].cpu().numpy().view(np.uint32)
    assert (after <= before).all() and (after < before).any() and after.sum() > 0

    # a flip applied twice gives back the canonical runs
    once = D.rle_flip(pair_g, sizes, horizontal=True, vertical=True)
    twice = D.rle_flip(once[0], once[3], horizontal=True, vertical=True)
    canonical = D.rle_flip_host(pair_h, sizes)                                                 # the identity record: the canonical RLE of every plane
    same(twice, canonical, "resident, flip twice")
    assert (once[1].cpu().numpy() == twice[1].cpu().numpy()).all() and (once[0][0].cpu().numpy().tolist() != twice[0][0].cpu().numpy().tolist())

    # the resized pair handed on to the polygon and the drawing entries, against the host route from the same runs
    small = [(h // 4, w // 4) for h, w in sizes]
    res_g = D.rle_resize(pair_g, sizes, small)
    res_h = D.rle_resize_host(pair_h, sizes, small)
    same(res_g, res_h, "resident, resize")
    rings = D.rle_to_polygons(res_g[0], res_g[3], flat=True)
    assert rings["xy"].is_cuda
    rings_h = D.rle_to_polygons_host(res_h[0], res_h[3], flat=True)
    for key in ("rle_rings", "ring_offsets", "ring_areas", "xy"):
        assert (rings[key].cpu().numpy() == rings_h[key]).all(), key
    planes = D.rle_decode_planes(res_g[0], res_g[3])
    planes_h = D.rle_decode_planes_host(res_h[0], res_h[3])
    for b in range(len(sizes)):
        assert planes[b].is_cuda and planes[b].shape[1:] == small[b] and (planes[b].cpu().numpy() == planes_h[b]).all(), b
    # and a quarter turn of the resident pair, transposed records on real masks
    same(D.rle_rot90(pair_g, sizes, 1), D.rle_rot90_host(pair_h, sizes, 1), "resident, rot90")
