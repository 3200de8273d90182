"""k_roi_align_nhwc (csrc/kernels_roialign.hip) outside the one shape the engine runs it at (C = 256, P = 7 | 14).

The kernel has an 8-channel item path (fp16, C % 8 == 0) and a 4-channel one, a shift / mask item index when the items per point
are a power of two and a divide otherwise, one pass over a 256-entry LDS table of sampled points per 256 points of P * P, a per-level
power-of-two multiplier, and the removeZeros predicate reduced over the fp32 values before the store rounds them.  Every comparison
here is bit for bit against the CPU oracle (oracle/mrcnn_oracle.c), which states the same fp32 arithmetic sample by sample:

  fp32   the oracle on the maps transposed to CHW;
  fp16   the oracle on the fp16 maps widened to fp32, rounded ONCE to fp16 (numpy astype: round-to-nearest-even, subnormals kept);
  flags  1 exactly for the rows orc.mask_valid_rows keeps of the fp32 samples, in both dtypes.

The public entry mrcnn_roi_align_nhwc reaches one image with multipliers 1; the batch strides and the multipliers are reached through
the test entry mrcnn_test_roi_align_nhwc_batch (include/maskrcnn_hip_test.h).
"""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")

CHANNELS = (4, 8, 12, 20, 24, 40, 64, 256)
POOLS = (1, 2, 7, 14, 16, 17, 28)          # 16: the 256-entry table exactly full; 17: a second pass of 33 points; 28: four passes, the last of 16
N_ROIS = (1, 3, 130)
ROI_STRIDES = (4, 5, 6)
# level sizes (H, W) of the four maps and the image (w, h) the ROI levels are computed for
PYRAMIDS = {
    "square": (((32, 32), (16, 16), (8, 8), (4, 4)), (1024.0, 1024.0)),
    "wide": (((32, 64), (16, 32), (8, 16), (4, 8)), (2048.0, 1024.0)),
    "tall_odd": (((24, 10), (12, 5), (6, 3), (3, 2)), (512.0, 1024.0)),
    "top_1x1": (((8, 8), (4, 4), (2, 2), (1, 1)), (1024.0, 1024.0)),
}
NP_DTYPE = {"f32": np.float32, "f16": np.float16}
LIB_DTYPE = {"f32": L.F32, "f16": L.F16}
# the rows every kernel of this family has gone wrong on at some point (levels for a 1024 x 1024 image in the comments)
EDGE_ROIS = np.array([
    [0.0, 0.0, 0.0, 0.0],                  # all-zero padding row                                   -> level -1
    [0.3, 0.3, 0.3, 0.3],                  # zero area: log2(0) = -inf                              -> -1
    [0.5, 0.5, 0.4, 0.6],                  # singly inverted: sqrt of a negative area is NaN        -> -1
    [0.6, 0.7, 0.4, 0.5],                  # doubly inverted: the area is positive, sampled backwards -> 2
    [0.0, 0.0, 1.0, 1.0],                  # the whole image                                        -> 3
    [1.0, 1.0, 1.001, 1.001],              # on the far border: the first sample is the last pixel  -> 0
    [-0.1, 0.8, 0.3, 1.2],                 # partly outside
    [1.2, 1.3, 1.5, 1.6],                  # wholly outside, beyond the far edges
    [-0.6, -0.5, -0.2, -0.1],              # wholly outside, before the near edges
    [-0.5, -0.5, 1.5, 1.5],                # larger than the image
    [0.20, 0.20, 0.25, 0.26],              # inside                                                 -> 0
    [0.10, 0.10, 0.20, 0.22],              # inside                                                 -> 1
    [0.30, 0.30, 0.50, 0.52],              # inside                                                 -> 2
    [0.05, 0.10, 0.90, 0.95],              # inside                                                 -> 3
], np.float32)


def _paths(dtype, channels, pool):
    """(item path, index path, passes) the kernel takes: its own rules restated (kernels_roialign.hip: `wide`, `pow2`, the p0 loop)."""
    wide = dtype == "f16" and channels % 8 == 0
    items = channels // 8 if wide else channels // 4
    return ("wide" if wide else "quad", "shift" if items & (items - 1) == 0 else "divide", (pool * pool + 255) // 256)


def _make_rois(rng, n, stride, first_edge):
    """n rows of `stride` floats: the edge rows first (n < their count: a window of them starting at first_edge), random boxes — tiny to larger than the
    image, some starting outside it — behind them; the columns past the fourth hold a value no box holds."""
    rows = np.full((n, stride), np.float32(777.0), np.float32)
    y1 = rng.random(n) * 1.2 - 0.1
    x1 = rng.random(n) * 1.2 - 0.1
    hh = rng.random(n) ** 3 * 1.1
    ww = rng.random(n) ** 3 * 1.1
    rows[:, :4] = np.stack([y1, x1, y1 + hh, x1 + ww], 1).astype(np.float32)
    k = min(n, len(EDGE_ROIS))
    rows[:k, :4] = EDGE_ROIS[(first_edge + np.arange(k)) % len(EDGE_ROIS)]
    return rows


def _make_maps(rng, sizes, channels, dtype, batch=None):
    """NHWC maps in the kernel's dtype, (batch,) H, W, C."""
    lead = () if batch is None else (batch,)
    return [rng.standard_normal(lead + (h, w, channels)).astype(np.float32).astype(NP_DTYPE[dtype]) for h, w in sizes]


def _chw32(m):
    return np.ascontiguousarray(m.astype(np.float32).transpose(2, 0, 1))


def _expected(orc, maps, rois, pool, img, dtype, level_mul=None):
    """(out (n, P, P, C) in the kernel's dtype, flags (n,) int32, fp32 values (n, C, P, P)) from the oracle; level_mul: the fp32 sample times
    float32(mul[level of the ROI]) — one fp32 rounding, as the kernel's `v * mul`."""
    r4 = np.ascontiguousarray(rois[:, :4])
    v32 = orc.pyramid_roi_align(r4, [_chw32(m) for m in maps], pool, img[0], img[1])
    if level_mul is not None:
        lv = orc.roi_levels(r4, img[0], img[1])
        mul = np.asarray(level_mul, np.float32)[np.maximum(lv, 0)]          # (a padding row is all zeros whatever it is multiplied by)
        v32 = v32 * mul[:, None, None, None]
        assert v32.dtype == np.float32
    assert np.isfinite(v32).all()
    flags = np.zeros(rois.shape[0], np.int32)
    flags[orc.mask_valid_rows(v32)] = 1
    out = np.ascontiguousarray(v32.transpose(0, 2, 3, 1)).astype(NP_DTYPE[dtype])
    return out, flags, v32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _assert_same_bits(got, want, msg=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def _level_args(maps, spatial_axis=0):
    hs = (C.c_int * 4)(*[m.shape[spatial_axis] for m in maps])
    ws = (C.c_int * 4)(*[m.shape[spatial_axis + 1] for m in maps])
    return hs, ws


def _public(maps, channels, dtype, rois, pool, img, want_flags=True):
    """mrcnn_roi_align_nhwc on host arrays -> (out, flags | None).  The output starts as NaN and the flags as -1: nothing may be left unwritten."""
    n, stride = rois.shape
    hs, ws = _level_args(maps)
    ptrs = (C.c_void_p * 4)(*[m.ctypes.data for m in maps])
    out = np.full((n, pool, pool, channels), np.nan, NP_DTYPE[dtype])
    flags = np.full(n, -1, np.int32) if want_flags else None
    L.check(L.lib().mrcnn_roi_align_nhwc(ptrs, hs, ws, channels, LIB_DTYPE[dtype], rois.ctypes.data, stride, n, pool, img[0], img[1], L.HOST,
                                         out.ctypes.data, flags.ctypes.data if want_flags else None))
    return out, flags


def _grid_cases():
    """Every C with every P; n_rois, roi_stride and the pyramid rotate so that each value meets each path.  (C = 256, P = 28) gets n_rois = 130."""
    keys = list(PYRAMIDS)
    for ic, channels in enumerate(CHANNELS):
        for ip, pool in enumerate(POOLS):
            yield channels, pool, N_ROIS[(ic + ip + 1) % 3], ROI_STRIDES[(ic + 2 * ip) % 3], keys[(ic * len(POOLS) + ip) % len(keys)]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_grid_through_the_public_entry(orc, dtype):
    """Every channel count x every pool size, bit for bit, with the paths the kernel took counted and all of them required."""
    seen_paths, seen_levels, seen_values = set(), set(), {"n": set(), "stride": set(), "pyramid": set()}
    for case, (channels, pool, n, stride, key) in enumerate(_grid_cases()):
        sizes, img = PYRAMIDS[key]
        rng = np.random.default_rng(9000 + case)
        maps = _make_maps(rng, sizes, channels, dtype)
        rois = _make_rois(rng, n, stride, first_edge=case)
        want, want_flags, _ = _expected(orc, maps, rois, pool, img, dtype)
        got, flags = _public(maps, channels, dtype, rois, pool, img)
        msg = f"{dtype} C={channels} P={pool} n={n} roi_stride={stride} pyramid={key}"
        _assert_same_bits(got, want, msg)
        np.testing.assert_array_equal(flags, want_flags, err_msg=msg)
        if n >= 64:       # a condition of the case, not a hope: a kept and a dropped row are both in it
            assert set(np.unique(want_flags).tolist()) == {0, 1}, msg
        seen_paths.add(_paths(dtype, channels, pool))
        seen_levels |= set(np.unique(orc.roi_levels(np.ascontiguousarray(rois[:, :4]), img[0], img[1])).tolist())
        seen_values["n"].add(n); seen_values["stride"].add(stride); seen_values["pyramid"].add(key)
    item_paths = ("wide", "quad") if dtype == "f16" else ("quad",)          # fp32 has no 8-channel items
    required = {(i, x, p) for i in item_paths for x in ("shift", "divide") for p in (1, 2, 4)}
    assert seen_paths == required, (dtype, sorted(required - seen_paths), sorted(seen_paths - required))
    assert seen_levels >= {-1, 0, 1, 2, 3}
    assert seen_values == {"n": set(N_ROIS), "stride": set(ROI_STRIDES), "pyramid": set(PYRAMIDS)}


def test_edge_rows_are_what_their_comments_say(orc):
    """The fixture itself: which of EDGE_ROIS are padding, and that the doubly inverted one is a valid level sampled backwards (non-zero output)."""
    lv = orc.roi_levels(EDGE_ROIS, 1024.0, 1024.0)
    assert lv[:6].tolist() == [-1, -1, -1, 2, 3, 0] and lv[10:].tolist() == [0, 1, 2, 3]
    sizes, img = PYRAMIDS["square"]
    maps = _make_maps(np.random.default_rng(1), sizes, 4, "f32")
    _, flags, v = _expected(orc, maps, EDGE_ROIS, 7, img, "f32")
    assert (v[3] != 0).all() and flags[3] == 1                             # doubly inverted: every sample inside the image
    assert (v[[0, 1, 2, 7, 8]] == 0).all()                                 # padding rows and boxes wholly outside
    assert (v[6] != 0).any() and (v[6] == 0).any() and (v[9] != 0).any() and (v[9] == 0).any()      # partly outside, larger than the image
    assert (v[5] != 0).any() and flags[5] == 0                              # far border: the corner sample reads the last pixel
    assert flags[10:].tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_one_planted_zero_drops_exactly_its_row(orc, dtype):
    """A row is dropped for ONE zero element: a 2 x 2 patch of zeros in one channel of P2 under one sample point of an ROI inside the image
    (P = 3, samples 1.18 pixels apart: each in a cell of its own, only the centre one has all four corners in the patch).  C = 12: the divide path."""
    channels, pool, ch0 = 12, 3, 5
    sizes, img = PYRAMIDS["square"]
    maps = _make_maps(np.random.default_rng(42), sizes, channels, dtype)
    maps[0][10:12, 13:15, ch0] = 0
    # y: 0.300 * 31 = 9.3, 10.478, 11.656; x: 0.400 * 31 = 12.4, 13.578, 14.756 -> the centre sample lies in cell (10, 13); sqrt(area) = 0.076 -> level 0
    rois = np.array([[0.300, 0.400, 0.376, 0.476],
                     [0.300, 0.600, 0.376, 0.676]], np.float32)            # the neighbour: the same box 6.2 pixels to the right
    want, want_flags, v32 = _expected(orc, maps, rois, pool, img, dtype)
    assert orc.roi_levels(rois, *img).tolist() == [0, 0]
    assert int((v32[0] == 0).sum()) == 1 and v32[0, ch0, 1, 1] == 0 and int((v32[1] == 0).sum()) == 0
    assert want_flags.tolist() == [0, 1]
    got, flags = _public(maps, channels, dtype, rois, pool, img)
    _assert_same_bits(got, want)
    assert flags.tolist() == [0, 1]
    # without the flags the same output
    got2, _ = _public(maps, channels, dtype, rois, pool, img, want_flags=False)
    _assert_same_bits(got2, want)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_null_row_flags_write_the_same_output(orc, dtype):
    """row_flags = NULL at a multi-pass shape (the flag reduction is the only barrier behind the last pass)."""
    channels, pool = 20, 17
    sizes, img = PYRAMIDS["wide"]
    rng = np.random.default_rng(77)
    maps = _make_maps(rng, sizes, channels, dtype)
    rois = _make_rois(rng, 20, 5, 0)
    want, want_flags, _ = _expected(orc, maps, rois, pool, img, dtype)
    got, flags = _public(maps, channels, dtype, rois, pool, img)
    got2, none = _public(maps, channels, dtype, rois, pool, img, want_flags=False)
    assert none is None
    _assert_same_bits(got, want)
    _assert_same_bits(got2, want)
    np.testing.assert_array_equal(flags, want_flags)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("channels,pool", [(24, 17), (12, 28), (40, 14)])
def test_device_memory_in_place(orc, dtype, channels, pool):
    """MRCNN_DEVICE: the kernel reads the caller's tensors and writes the caller's output where it lies — a slice with sentinel-filled guards before
    and behind it, which must stay untouched, as must the maps and the ROIs.  (24, 17): two passes, divide (fp16: 8-channel items); (12, 28): four
    passes, divide, 4-channel items; (40, 14): one pass, divide."""
    import torch
    tdt = {"f32": torch.float32, "f16": torch.float16}[dtype]
    sizes, img = PYRAMIDS["tall_odd"]
    rng = np.random.default_rng(500 + channels + pool)
    n, stride = 70, 4
    maps = _make_maps(rng, sizes, channels, dtype)
    rois = _make_rois(rng, n, stride, 0)
    want, want_flags, _ = _expected(orc, maps, rois, pool, img, dtype)
    assert set(np.unique(want_flags).tolist()) == {0, 1}
    maps_d = [torch.from_numpy(m).cuda() for m in maps]
    rois_d = torch.from_numpy(rois).cuda()
    guard, fguard, sentinel = 64, 4, 1234.0       # 64 elements: the slice keeps the 16-byte alignment of the kernel's vector stores
    row = pool * pool * channels
    buf = torch.full((guard + n * row + guard,), sentinel, dtype=tdt, device="cuda")
    fbuf = torch.full((fguard + n + fguard,), -7, dtype=torch.int32, device="cuda")
    out_d, flags_d = buf[guard:guard + n * row], fbuf[fguard:fguard + n]
    assert out_d.data_ptr() % 16 == 0 and all(m.data_ptr() % 16 == 0 for m in maps_d)
    torch.cuda.synchronize()                      # the library runs on a stream of its own
    hs, ws = _level_args(maps)
    ptrs = (C.c_void_p * 4)(*[m.data_ptr() for m in maps_d])
    L.check(L.lib().mrcnn_roi_align_nhwc(ptrs, hs, ws, channels, LIB_DTYPE[dtype], rois_d.data_ptr(), stride, n, pool, img[0], img[1], L.DEVICE,
                                         out_d.data_ptr(), flags_d.data_ptr()))
    got = buf.cpu().numpy()
    gflags = fbuf.cpu().numpy()
    _assert_same_bits(got[guard:guard + n * row].reshape(want.shape), want)
    np.testing.assert_array_equal(gflags[fguard:fguard + n], want_flags)
    assert (got[:guard] == sentinel).all() and (got[guard + n * row:] == sentinel).all()
    assert (gflags[:fguard] == -7).all() and (gflags[fguard + n:] == -7).all()
    for m_d, m in zip(maps_d, maps):
        _assert_same_bits(m_d.cpu().numpy(), m)
    _assert_same_bits(rois_d.cpu().numpy(), rois)


@pytest.mark.parametrize("channels,pool,key", [(12, 7, "wide"), (64, 17, "tall_odd"), (8, 28, "top_1x1")])
def test_nhwc_kernel_and_the_layers_kernel_give_the_same_bits(pkg, orc, channels, pool, key):
    """k_roi_align_nhwc against k_roi_align_nchw (PyramidROIAlignLayer) on the same data: the two share make_sample and nothing else."""
    sizes, img = PYRAMIDS[key]
    rng = np.random.default_rng(600 + channels)
    n = 60
    maps = _make_maps(rng, sizes, channels, "f32")
    rois = _make_rois(rng, n, 4, 0)
    got, _ = _public(maps, channels, "f32", rois, pool, img)
    fm = [_chw32(m) for m in maps]
    layer = pkg.PyramidROIAlignLayer({"poolSize": pool, "imageWidth": int(img[0]), "imageHeight": int(img[1])})
    ML = pkg.MLMultiArray
    out = np.full((n, 1, channels, pool, pool), np.float32(np.nan), np.float32)
    layer.evaluate([ML(rois)] + [ML(f) for f in fm], [ML(out)])
    _assert_same_bits(np.ascontiguousarray(got.transpose(0, 3, 1, 2)), out.reshape(n, channels, pool, pool))
    _assert_same_bits(out.reshape(n, channels, pool, pool), orc.pyramid_roi_align(rois, fm, pool, img[0], img[1]))


def test_argument_handling():
    """What the entry decides on the host, before any launch."""
    channels, pool, n = 8, 2, 3
    sizes, img = PYRAMIDS["square"]
    rng = np.random.default_rng(3)
    maps = _make_maps(rng, sizes, channels, "f32")
    rois = _make_rois(rng, n, 4, 10)
    hs, ws = _level_args(maps)
    ptrs = (C.c_void_p * 4)(*[m.ctypes.data for m in maps])
    out = np.full((n, pool, pool, channels), np.float32(-5.0), np.float32)
    flags = np.full(n, -1, np.int32)

    def call(ptrs=ptrs, hs=hs, channels=channels, dtype=L.F32, stride=4, n=n, pool=pool):
        return L.lib().mrcnn_roi_align_nhwc(ptrs, hs, ws, channels, dtype, rois.ctypes.data, stride, n, pool, img[0], img[1], L.HOST, out.ctypes.data,
                                            flags.ctypes.data)
    INVALID, UNSUPPORTED = 1, 5
    assert call(n=0) == L.MRCNN_OK
    assert (out == -5.0).all() and (flags == -1).all()
    assert call(channels=6) == INVALID
    assert call(channels=0) == INVALID
    assert call(pool=0) == INVALID
    assert call(stride=3) == INVALID
    assert call(dtype=L.F32S) == UNSUPPORTED
    assert call(dtype=L.F32X3) == UNSUPPORTED
    no_p4 = (C.c_void_p * 4)(maps[0].ctypes.data, maps[1].ctypes.data, None, maps[3].ctypes.data)
    assert call(ptrs=no_p4) == INVALID
    assert b"level 2 missing" in L.lib().mrcnn_last_error()
    no_h = (C.c_int * 4)(32, 0, 8, 4)
    assert call(hs=no_h) == INVALID
    assert (out == -5.0).all() and (flags == -1).all()                     # none of the refused calls wrote anything
    assert call() == L.MRCNN_OK and not (out == -5.0).any() and set(flags.tolist()) <= {0, 1}


# ---------------------------------------------------------------------------------------------------------------------
# batch strides and level multipliers: mrcnn_test_roi_align_nhwc_batch
# ---------------------------------------------------------------------------------------------------------------------
LEVEL_MUL = (8.0, 1.0, 0.25, 32.0)                # 2^3, 1, 2^-2, 2^5
TINY = np.float32(2.0 ** -24)                     # the smallest positive fp16 subnormal


def _batch_entry(maps, channels, dtype, level_mul, rois, pool, img, want_flags=True):
    """maps[l] (B, H, W, C) in the kernel's dtype (handed over widened: the entry rounds to `dtype` again, exactly); rois (B, n, stride)."""
    batch, n, stride = rois.shape
    m32 = [np.ascontiguousarray(m.astype(np.float32)) for m in maps]
    hs, ws = _level_args(maps, 1)
    ptrs = (C.c_void_p * 4)(*[m.ctypes.data for m in m32])
    mul = (C.c_float * 4)(*level_mul)
    out = np.full((batch, n, pool, pool, channels), np.nan, np.float32)
    flags = np.full((batch, n), -1, np.int32) if want_flags else None
    L.check(L.lib().mrcnn_test_roi_align_nhwc_batch(ptrs, hs, ws, channels, LIB_DTYPE[dtype], mul, rois.ctypes.data, stride, n, batch, pool, img[0], img[1],
                                                    out.ctypes.data, flags.ctypes.data if want_flags else None))
    return out, flags


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("channels,pool", [(12, 7), (12, 17), (64, 7), (64, 17)])
def test_batch_strides_and_level_multipliers(orc, dtype, channels, pool):
    """Three images with maps and ROIs of their own in one launch, the four levels at four different powers of two.  Expected, per image: the oracle's
    fp32 sample times float32(mul[level]) (rounded once for fp16), flags from that fp32 product.  Image 1's P4 holds the smallest fp16 subnormal
    everywhere (as test_roi_align_fp16_tiny_samples_keep_their_rows builds its maps): times 2^-2 the samples of an ROI on that level are non-zero in
    fp32 — the row is kept — and zero once stored as fp16, while the unscaled samples would have been stored non-zero."""
    batch, n, stride, tiny_img, tiny_level, tiny_row = 3, 40, 5, 1, 2, 12
    sizes, img = PYRAMIDS["wide"]
    rng = np.random.default_rng(800 + channels + pool)
    maps = _make_maps(rng, sizes, channels, dtype, batch)
    maps[tiny_level][tiny_img] = TINY
    rois = np.stack([_make_rois(rng, n, stride, 0) for _ in range(batch)])
    rois[:, tiny_row, :4] = [0.30, 0.30, 0.45, 0.50]                       # inside the image; sqrt(area) = 0.173, image 2048 x 1024 -> level 2
    want, want_flags, v32 = zip(*[_expected(orc, [m[b] for m in maps], rois[b], pool, img, dtype, LEVEL_MUL) for b in range(batch)])
    # the fixture, confirmed on the CPU before the GPU runs
    lv = [orc.roi_levels(np.ascontiguousarray(rois[b, :, :4]), *img) for b in range(batch)]
    assert lv[tiny_img][tiny_row] == tiny_level and LEVEL_MUL[tiny_level] == 0.25
    assert set(np.unique(np.concatenate(lv)).tolist()) >= {-1, 0, 1, 2, 3}
    unscaled = _expected(orc, [m[tiny_img] for m in maps], rois[tiny_img], pool, img, dtype)[2][tiny_row]
    assert (unscaled == TINY).all() and (unscaled.astype(np.float16) != 0).all()
    assert (v32[tiny_img][tiny_row] == TINY * np.float32(0.25)).all() and want_flags[tiny_img][tiny_row] == 1
    if dtype == "f16":
        assert (want[tiny_img][tiny_row] == 0).all()
    for b in range(batch):
        assert set(np.unique(want_flags[b]).tolist()) == {0, 1}
    assert not np.array_equal(rois[0], rois[1]) and not np.array_equal(maps[0][0], maps[0][2])
    got, flags = _batch_entry(maps, channels, dtype, LEVEL_MUL, rois, pool, img)
    for b in range(batch):
        _assert_same_bits(got[b], want[b].astype(np.float32), f"image {b}")
        np.testing.assert_array_equal(flags[b], want_flags[b], err_msg=f"image {b}")
        # image b of the batch = the same data run alone
        one, one_flags = _batch_entry([m[b:b + 1] for m in maps], channels, dtype, LEVEL_MUL, rois[b:b + 1], pool, img)
        _assert_same_bits(got[b], one[0], f"image {b} alone")
        np.testing.assert_array_equal(flags[b], one_flags[0])
    no_flags, none = _batch_entry(maps, channels, dtype, LEVEL_MUL, rois, pool, img, want_flags=False)
    assert none is None
    _assert_same_bits(no_flags, got)
