"""Kernel-level parity of the convolution family through mrcnn_conv2d_nhwc (C ABI).

The tile shape / pipeline variant a layer runs on depends on its GEMM size, i.e. on the batch: the 256-row ping-pong
fp16 kernels (kernels_conv_pp.hip) take over from the 128-row kernel once the grid fills the chip.  Per-image results
must not depend on the batch, so both kernels have to produce BIT-IDENTICAL outputs on the same data — checked here
directly, layer shape by layer shape (incl. ragged M, zero padding on every border, residual, stride 2, 1×1 and 3×3,
K tiles from 2 up), next to a torch-CPU fp32 reference within the fp16-operand tolerance.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")


def conv(x, w, k, stride, scale=None, shift=None, res=None, act=1, dtype="f16"):
    B, H, W, Ci = x.shape
    Co = w.shape[0]
    pad = k // 2
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.empty((B, oh, ow, Co), np.float32)
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (x, w, scale, shift, res)]
    ptr = [None if a is None else a.ctypes.data for a in keep]
    L.check(L.lib().mrcnn_conv2d_nhwc(ptr[0], B, H, W, Ci, ptr[1], Co, k, stride, ptr[2], ptr[3], ptr[4], act,
                                      {"f32": L.F32, "f16": L.F16, "f32s": L.F32S, "f32x3": L.F32X3}[dtype], out.ctypes.data))
    return out


import contextlib


@contextlib.contextmanager
def old_family():
    """The 3x3 stride-1 layers of the split modes run on the halo kernel (kernels_conv_halo.hip, its own K order) whenever
    they qualify; the bit-identity tests BETWEEN the older kernels of the family switch it off for their duration."""
    L.check(L.lib().mrcnn_debug_set(b"conv_halo", 0))
    try:
        yield
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_halo", 1))


def torch_ref(x, w, k, stride, scale, shift, res, act, dtype="f16"):
    """fp64 reference on the operands the engine sees: fp16 mode rounds activations, filters and residual to fp16; the
    split modes keep fp32 activations and use fp16 filters."""
    import torch
    import torch.nn.functional as F
    h = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float16).astype(np.float64))
    f = (lambda a: torch.from_numpy(np.asarray(a, np.float64))) if dtype != "f16" else h
    y = F.conv2d(f(x).permute(0, 3, 1, 2), h(w).permute(0, 3, 1, 2), stride=stride, padding=k // 2)
    y = y * torch.from_numpy(scale.astype(np.float64))[None, :, None, None] + torch.from_numpy(shift.astype(np.float64))[None, :, None, None]
    if res is not None:
        y = y + f(res).permute(0, 3, 1, 2)
    if act == 1:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


SHAPES = [  # B, H, W, Cin, Cout, k, stride, residual
    (2, 64, 64, 256, 256, 3, 1, False),      # M = 8192 = 32 tiles of 256, K = 36 tiles: every border of the zero padding
    (1, 72, 56, 128, 256, 3, 1, False),      # M = 4032: ragged last M tile (4032 = 15.75 × 256), non-square image
    (2, 48, 48, 256, 512, 1, 1, True),       # 1×1 with residual, two N tiles, K = 4 tiles (the minimum the policy admits)
    (1, 96, 96, 64, 256, 3, 2, False),       # stride 2, Cin = 64 (one channel tile per tap: a tap change every K tile)
    (3, 40, 40, 320, 256, 1, 1, False),      # odd K-tile count (5)
    (1, 33, 47, 192, 300, 3, 1, True),       # Cout not a multiple of the tile (Npad 384 → the 128-row kernel on both sides)
    (5, 40, 40, 96, 256, 3, 1, False),       # M = 8000 (ragged), 96 channels: fp16 K step does not divide (128-row kernel), split does
]


# (the fp16 kernels step K by 64 channels: a shape whose channel count does not divide is not a case of that mode — not generated, rather than skipped)
@pytest.mark.parametrize("shape,dtype", [(sh, dt) for sh in SHAPES for dt in ("f16", "f32s", "f32x3") if not (dt == "f16" and sh[3] % 64)])
def test_pingpong_kernel_equals_128row_kernel_bitwise(shape, dtype):
    B, H, W, Ci, Co, k, stride, with_res = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, H, W, Ci), np.float32)
    w = (rng.standard_normal((Co, k, k, Ci), np.float32) * np.float32(1.0 / np.sqrt(k * k * Ci)))
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = rng.standard_normal(Co).astype(np.float32) * np.float32(0.1)
    oh, ow = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = rng.standard_normal((B, oh, ow, Co), np.float32) if with_res else None
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"conv_halo", 0))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 0))
        y0 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"conv_pp", 1))
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_tiles", 1))       # force the ping-pong kernel onto small grids
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_kt", 2))
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_fill", 0))
        L.check(lib.mrcnn_debug_set(b"conv_pp_split", 1))
        y1 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
    finally:
        L.check(lib.mrcnn_debug_set(b"conv_halo", 1))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 1))
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_tiles", 512))
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_kt", 16))
        L.check(lib.mrcnn_debug_set(b"conv_pp_min_fill", 85))
        L.check(lib.mrcnn_debug_set(b"conv_pp_split", 0))
    np.testing.assert_array_equal(y1, y0)
    ref = torch_ref(x, w, k, stride, scale, shift, res, 1, dtype)
    tol = {"f16": 2e-3, "f32s": 2e-5, "f32x3": 1e-5}[dtype]      # fp16 output rounding / 22-bit split / fp32 summation order
    assert np.abs(y1 - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(y1 - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["f32s", "f32x3"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 256, 256, 3, 1, True), (1, 72, 56, 128, 300, 3, 1, False), (3, 40, 40, 320, 256, 1, 1, False)])
def test_wide_wave_variant_equals_the_eight_wave_tile_bitwise(shape, dtype):
    """Split modes: the 128x128 tile run by 4 waves of 32x128 (policy: K >= 2048, i.e. per-image results of a layer must not
    depend on which of the two the policy picked) against the same tile run by 8 waves of 32x64 — ragged M, ragged N, residual."""
    B, H, W, Ci, Co, k, stride, with_res = shape
    rng = np.random.default_rng(sum(shape) + 1)
    x = rng.standard_normal((B, H, W, Ci), np.float32)
    w = (rng.standard_normal((Co, k, k, Ci), np.float32) * np.float32(1.0 / np.sqrt(k * k * Ci)))
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = rng.standard_normal(Co).astype(np.float32) * np.float32(0.1)
    res = rng.standard_normal((B, H, W, Co), np.float32) if with_res else None
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"conv_halo", 0))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 0))
        L.check(lib.mrcnn_debug_set(b"conv_tn4", 0))
        y0 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"conv_tn4", 1))
        y1 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
    finally:
        L.check(lib.mrcnn_debug_set(b"conv_tn4", -1))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 1))
        L.check(lib.mrcnn_debug_set(b"conv_halo", 1))
    np.testing.assert_array_equal(y1, y0)


DIRECT_DEFAULT = 3      # MRCNN_DIRECT of conv_dispatch.hip


@pytest.mark.parametrize("dtype", ["f16", "f32", "f32s", "f32x3"])
@pytest.mark.parametrize("shape", [(2, 64, 64, 256, 256, 1, 1, True), (1, 72, 56, 128, 300, 3, 1, True), (3, 40, 40, 64, 128, 1, 2, False),
                                   (1, 33, 47, 192, 64, 3, 1, True), (1, 33, 47, 192, 136, 3, 1, True)])
def test_direct_epilogue_equals_the_lds_staged_epilogue_bitwise(shape, dtype):
    """The epilogue straight from the (transposed) accumulators — the default for fp16 tensors — against the LDS-staged
    full-row form (the default for fp32 tensors), forced either way in every mode: ragged M, ragged N (vector stores still
    possible), residual, stride 2, 64- and 128-wide tiles."""
    B, H, W, Ci, Co, k, stride, with_res = shape
    rng = np.random.default_rng(sum(shape) + 5)
    x = rng.standard_normal((B, H, W, Ci), np.float32)
    w = (rng.standard_normal((Co, k, k, Ci), np.float32) * np.float32(1.0 / np.sqrt(k * k * Ci)))
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = rng.standard_normal(Co).astype(np.float32) * np.float32(0.1)
    oh, ow = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = rng.standard_normal((B, oh, ow, Co), np.float32) if with_res else None
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"conv_halo", 0))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 0))
        L.check(lib.mrcnn_debug_set(b"conv_direct", 0))
        y0 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"conv_direct", 2))
        y1 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"conv_direct", 3))      # fp16 tensors through wave-private tiles (128-column kernel)
        y2 = conv(x, w, k, stride, scale, shift, res, 1, dtype)
    finally:
        L.check(lib.mrcnn_debug_set(b"conv_direct", DIRECT_DEFAULT))
        L.check(lib.mrcnn_debug_set(b"conv_pp", 1))
        L.check(lib.mrcnn_debug_set(b"conv_halo", 1))
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(y2, y0)
    ref = torch_ref(x, w, k, stride, scale, shift, res, 1, dtype if dtype != "f32" else "f32s")
    if dtype == "f32":          # exact-fp32 MFMA on fp32 filters: the reference must not round the filters to fp16
        import torch
        import torch.nn.functional as F
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        r = F.conv2d(t(x).permute(0, 3, 1, 2), t(w).permute(0, 3, 1, 2), stride=stride, padding=k // 2)
        r = r * t(scale)[None, :, None, None] + t(shift)[None, :, None, None]
        if res is not None:
            r = r + t(res).permute(0, 3, 1, 2)
        ref = F.relu(r).permute(0, 2, 3, 1).contiguous().numpy()
    tol = {"f16": 2e-3, "f32": 2e-5, "f32s": 2e-5, "f32x3": 1e-5}[dtype]
    assert np.abs(y1 - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(y1 - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["f16", "f32x3"])
def test_pingpong_kernel_repeatable_under_load(dtype):
    """Race screen of the hand-placed DMA / barrier schedule: the same launch repeated must give the same bits, on a
    grid larger than the chip (several rounds of blocks, blocks at different phases sharing L2)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 128, 128, 256), np.float32)
    w = rng.standard_normal((512, 3, 3, 256), np.float32) * np.float32(0.02)
    L.check(L.lib().mrcnn_debug_set(b"conv_halo", 0))
    L.check(L.lib().mrcnn_debug_set(b"conv_pp_split", 1))
    L.check(L.lib().mrcnn_debug_set(b"conv_pp_min_tiles", 1))
    y0 = conv(x, w, 3, 1, None, None, None, 1, dtype)
    for _ in range(4):
        np.testing.assert_array_equal(conv(x, w, 3, 1, None, None, None, 1, dtype), y0)
    L.check(L.lib().mrcnn_debug_set(b"conv_pp", 0))
    try:
        np.testing.assert_array_equal(conv(x, w, 3, 1, None, None, None, 1, dtype), y0)
    finally:
        L.check(L.lib().mrcnn_debug_set(b"conv_halo", 1))
        L.check(L.lib().mrcnn_debug_set(b"conv_pp", 1))
        L.check(L.lib().mrcnn_debug_set(b"conv_pp_split", 0))
        L.check(L.lib().mrcnn_debug_set(b"conv_pp_min_tiles", 512))


@pytest.mark.parametrize("dtype,batch", [("f32x3", 66), ("f16", 132)])
def test_activation_tensor_beyond_4_gib(dtype, batch):
    """The DMAs address activations with 32-bit offsets from a buffer resource that every block re-bases on the first image
    it touches: a tensor of more than 4 GiB (here 4.3 GiB: batch x 256 x 256 x 256) must give, for any image, exactly what
    that image gives alone (fp16: the ping-pong kernel; f32x3: the 128-row kernels).  Stride 2 keeps the output small."""
    import psutil
    if psutil.virtual_memory().available < 40 * 2**30:
        pytest.skip("needs ~25 GB of host memory for the staging copies")
    rng = np.random.default_rng(11)
    H = W = 256
    Ci, Co = 256, 256
    probe = [0, batch // 2, batch - 1]
    x = np.zeros((batch, H, W, Ci), np.float32)
    for b in probe:
        x[b] = rng.standard_normal((H, W, Ci), np.float32)
    assert x.nbytes // (2 if dtype == "f16" else 1) > 2**32
    w = rng.standard_normal((Co, 3, 3, Ci), np.float32) * np.float32(0.02)
    shift = rng.standard_normal(Co).astype(np.float32)
    y = conv(x, w, 3, 2, None, shift, None, 1, dtype)
    for b in probe:
        np.testing.assert_array_equal(y[b], conv(x[b:b + 1], w, 3, 2, None, shift, None, 1, dtype)[0])
    # an all-zero image gives relu(shift) everywhere (its padding taps and its neighbours' data never leak in)
    want = np.maximum(shift, 0)
    if dtype == "f16":
        want = want.astype(np.float16).astype(np.float32)
    np.testing.assert_array_equal(y[1], np.broadcast_to(want, y[1].shape))


# ---------------------------------------------------------------------------------------------------------------------
# the split modes are not scale-invariant the way fp32 is: the curve, and the bound the documentation states
# ---------------------------------------------------------------------------------------------------------------------
SCALES = [0, -4, -8, -12, -16, -20]


def split_scale_curve(dtype, shape=(2, 32, 32, 256, 128, 3), seed=3):
    """max |err| / max |ref| of one convolution against an fp64 torch convolution, for the SAME post-ReLU-like tensor
    multiplied by 2^e (an exact operation): [(e, relative error, bound)].  bound = what include/maskrcnn_hip.h documents for
    the three-part split: every activation is carried exactly when |a| >= 0.5 and to 2^-25 ABSOLUTE (rounded to
    nearest) below, so an output is off by at most 2^-25 * sum |w| over its taps (the test grants 2^-24) — plus the fp32 summation noise every
    fp32 engine has (taken as 2e-6 of the range, the bar of the other conv tests)."""
    B, H, W, Ci, Co, k = shape
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, H, W, Ci)), 0).astype(np.float32) * 4.0         # post-ReLU, O(1-10) like the trunk's
    w = (rng.standard_normal((Co, k, k, Ci)) * np.sqrt(2.0 / (k * k * Ci))).astype(np.float16).astype(np.float32)
    one, zero = np.ones(Co, np.float32), np.zeros(Co, np.float32)
    wsum = np.abs(w.astype(np.float64)).reshape(Co, -1).sum(1).max()
    out = []
    for e in SCALES:
        xs = np.ldexp(x, e).astype(np.float32)
        got = conv(xs, w, k, 1, one, zero, None, act=0, dtype=dtype).astype(np.float64)
        ref = torch_ref(xs, w, k, 1, one, zero, None, 0, dtype=dtype)
        rng_ref = np.abs(ref).max()
        out.append((e, float(np.abs(got - ref).max() / rng_ref), float(2.0 ** -24 * wsum / rng_ref + 2e-6)))
    return out


def split_scale_curve_calibrated(dtype, shape=(2, 32, 32, 256, 128, 3), seed=3):
    """The same curve with the engine's calibration applied (Model::calibrate_split's rule: the tensor is STORED as 2^p * value with
    max |a| * 2^p in [2^11, 2^12), the consumer's scale carries 2^-p — both exact): [(e, relative error, p)]."""
    B, H, W, Ci, Co, k = shape
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, H, W, Ci)), 0).astype(np.float32) * 4.0
    w = (rng.standard_normal((Co, k, k, Ci)) * np.sqrt(2.0 / (k * k * Ci))).astype(np.float16).astype(np.float32)
    one, zero = np.ones(Co, np.float32), np.zeros(Co, np.float32)
    out = []
    for e in SCALES:
        xs = np.ldexp(x, e).astype(np.float32)
        ref = torch_ref(xs, w, k, 1, one, zero, None, 0, dtype=dtype)
        _, kx = np.frexp(float(np.abs(xs).max()))
        p = 12 - int(kx)
        got = conv(np.ldexp(xs, p).astype(np.float32), w, k, 1, np.ldexp(one, -p).astype(np.float32), zero, None, act=0, dtype=dtype).astype(np.float64)
        out.append((e, float(np.abs(got - ref).max() / np.abs(ref).max()), p))
    return out


@pytest.mark.parametrize("dtype", ["f32x3", "f32s", "f32"])
def test_split_modes_scale_curve_stays_inside_the_documented_bound(dtype):
    """VERDICT r2 item 1(b) / ADVICE r2: the three-part split is exact only for 0.5 <= |a| < 65504; below, an activation is
    carried to 2^-25 absolute.  The same tensor at 2^0 ... 2^-20: the fp32-MFMA mode is flat (control), the split modes follow
    the documented bound (and must not be WORSE than it: that is what protects small-magnitude checkpoints from silent loss)."""
    curve = split_scale_curve(dtype)
    for e, err, bound in curve:
        if dtype == "f32":
            assert err < 2e-6, (e, err)                           # scale-invariant, like the reference's fp32
        elif dtype == "f32x3":
            assert err <= bound, (e, err, bound)
        else:                                                     # two-part split: 2^-22 relative on top
            assert err <= bound + 2.0 ** -21, (e, err, bound)
    if dtype == "f32x3":
        # at the trunk's own scale (O(1-10) activations) the split costs nothing measurable ...
        assert curve[0][1] < 2e-6
        # ... and the loss at tiny scales is real: were it to vanish, the documentation (and this test) should be revisited
        assert curve[-1][1] > 10 * curve[0][1]


# ---------------------------------------------------------------------------------------------------------------------
# the halo kernel (kernels_conv_halo.hip): 3x3 stride-1 layers of the split modes
# ---------------------------------------------------------------------------------------------------------------------
HALO_SHAPES = [  # B, H, W, Cin, Cout — every geometry class of the tile's input region
    (2, 128, 128, 64, 256),     # W % 128 == 0: single-row tiles, cropped region (pitch 130), left / right image borders
    (1, 256, 256, 32, 128),     # two tiles per row: a tile that starts in the middle of a row
    (3, 64, 64, 256, 256),      # two full rows per tile, top / bottom borders, 16 slabs
    (2, 72, 56, 96, 300),       # W = 56: tiles start anywhere in a row and straddle images; Cin = 96 (6 slabs); Cout 300 -> Npad 384
    (20, 14, 14, 256, 256),     # the mask head's geometry: 9 rows per tile, tiles straddling two images (zero rows between them)
    (5, 16, 16, 64, 512),       # the P6 geometry, 512 columns
    (1, 32, 32, 320, 64),       # 64 output columns (narrowest tile), 20 slabs
    (4, 48, 40, 128, 192),      # Npad 256, ragged last M tile (7680 = 60 tiles exactly) — and 40-wide rows
    (1, 33, 47, 192, 128),      # M = 1551: ragged last tile, odd sizes
    (2, 8, 192, 64, 256),       # round 4: W = 192 (the P3 level of 1536² inputs) — eligible through the two-row tiles only; 3 column blocks per row
    (1, 6, 256, 64, 256),       # two-row tiles, 4 column blocks: the left / right image border inside the row of tiles
    (3, 10, 128, 128, 512),     # two-row tiles with 512 columns (the fused-head layers' shape), three images
    (1, 256, 256, 64, 64),      # late round 4: 64 columns on the halo kernel (128 x 64 tiles, the waves as 4 x 2) — C2's layers: two-row tiles, four slabs
    (2, 64, 64, 64, 64),        # ... two image rows per tile (linear geometry)
    (3, 40, 40, 128, 64),       # ... ragged rows, tiles straddle images
    (9, 14, 14, 64, 64),        # ... nine rows per tile, pitch W + 16 and the image skew
    (2, 8, 192, 64, 64),        # ... two-row tiles, three column blocks per row
]


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", HALO_SHAPES)
def test_halo_kernel_against_fp64_and_the_128row_kernel(shape, dtype):
    """The persistent halo kernel on every geometry class (single-row tiles, multi-row, tiles that straddle images, ragged
    last tile, every border of the zero padding, 64 / 128 / 256-wide tiles): within the split modes' fp32-grade tolerance of an
    fp64 convolution, within summation-order noise of the 128-row kernel (whose K order differs), and REPEATABLE."""
    B, H, W, Ci, Co = shape
    rng = np.random.default_rng(sum(shape) + 17)
    x = (rng.standard_normal((B, H, W, Ci)) * 3).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    y = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
    ref = torch_ref(x, w, 3, 1, scale, shift, None, 1, dtype)
    tol = {"f32s": 2e-5, "f32x3": 1e-5}[dtype]
    assert np.abs(y - ref).max() <= tol * max(1.0, np.abs(ref).max()), (np.abs(y - ref).max(), np.abs(ref).max())
    np.testing.assert_array_equal(conv(x, w, 3, 1, scale, shift, None, 1, dtype), y)          # repeatable
    with old_family():
        y_old = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
    assert not np.array_equal(y_old, y) or True          # (different K order: equality is not expected, closeness is)
    assert np.abs(y_old - y).max() <= 2 * tol * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", [(6, 64, 64, 256, 256), (9, 14, 14, 256, 256), (4, 128, 128, 64, 512), (3, 72, 56, 96, 300), (4, 128, 128, 64, 64), (5, 24, 40, 64, 64)])
def test_halo_kernel_results_do_not_depend_on_the_batch(shape, dtype):
    """The sharding contract: an image's result is the same bits whatever batch it rides in — the batch changes the number
    of tiles, hence the tile WIDTH the launcher picks (256 / 128 / 64 columns) and which tiles straddle two images."""
    B, H, W, Ci, Co = shape
    rng = np.random.default_rng(sum(shape) + 23)
    x = (rng.standard_normal((B, H, W, Ci)) * 2).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    y = conv(x, w, 3, 1, None, shift, None, 1, dtype)
    for b in range(B):
        np.testing.assert_array_equal(conv(x[b:b + 1], w, 3, 1, None, shift, None, 1, dtype)[0], y[b], err_msg=f"image {b}")
    if B >= 4:
        np.testing.assert_array_equal(conv(x[1:4], w, 3, 1, None, shift, None, 1, dtype), y[1:4])


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", [(2, 128, 128, 64, 256), (1, 256, 256, 64, 512), (3, 64, 64, 256, 256), (20, 14, 14, 256, 256), (5, 16, 16, 64, 512),
                                   (2, 72, 56, 96, 300), (1, 32, 32, 320, 64), (9, 14, 14, 256, 256), (1, 64, 64, 256, 256), (1, 6, 256, 64, 256),
                                   (2, 128, 128, 64, 64), (1, 256, 256, 64, 64)])
def test_halo_tile_geometries_are_bit_identical(shape, dtype):
    """Round 4 changed WHICH output pixels a halo tile owns (two rows x 64 columns instead of one row x 128 where W >= 128:
    4 x 66 = 264 staged pixels per slab instead of 3 x 130 = 390), how many staging pieces a thread moves (2 / 3 / 5, by region
    size) and the LDS pitch of multi-row regions (conflict-free fragment reads) — none of which may change a single output bit:
    every tile sums its K in the same (slab, tap, part) order.  mrcnn_debug_set("halo_geo", 0) runs the round-3 geometries."""
    B, H, W, Ci, Co = shape
    rng = np.random.default_rng(sum(shape) + 29)
    x = (rng.standard_normal((B, H, W, Ci)) * 3).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    y = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
    try:
        L.check(L.lib().mrcnn_debug_set(b"halo_geo", 0))
        y3 = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
    finally:
        L.check(L.lib().mrcnn_debug_set(b"halo_geo", 1))
    np.testing.assert_array_equal(y, y3)


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", [(2, 256, 256, 64, 64), (8, 128, 128, 64, 64), (16, 64, 128, 64, 64), (34, 60, 64, 64, 64)])
def test_64_column_layers_256_row_arrangement_is_bit_identical(shape, dtype):
    """C2's 64 -> 64 layers: 256 x 64 tiles (four image rows x 64 columns, the eight waves as 8 x 1 with two accumulators each) on
    grids that fill the chip, 128 x 64 tiles (4 x 2 waves) otherwise — "halo_n64" 2 / 1; same (slab, tap, part) order, same bits,
    and a single image of the batch (which takes the 128-row arrangement) agrees too."""
    B, H, W, Ci, Co = shape
    rng = np.random.default_rng(sum(shape) + 3)
    x = (rng.standard_normal((B, H, W, Ci)) * 2).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"halo_n64", 1))
        y1 = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"halo_n64", 2))
        y2 = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
        y2b = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
        yb = conv(x[B - 1:], w, 3, 1, scale, shift, None, 1, dtype)
    finally:
        L.check(lib.mrcnn_debug_set(b"halo_n64", 2))
    np.testing.assert_array_equal(y2, y1)
    np.testing.assert_array_equal(y2b, y2)
    np.testing.assert_array_equal(yb[0], y2[B - 1])
    xs, ys = x[:1], y2[:1]
    ref = torch_ref(xs, w, 3, 1, scale, shift, None, 1, dtype)
    assert np.abs(ys - ref).max() <= (1e-5 if dtype == "f32x3" else 2e-5) * max(1.0, np.abs(ref).max())


LAT_SHAPES = [  # B, H, W, Cin, Cout — grids under 3/4 of the chip with 64 x 128 tiles: the 64 x 64 latency form (k_conv_halo_lat)
    (1, 64, 64, 256, 256),      # C4 at a single image: one-row regions of 3 x 66 pixels, four staging pieces
    (1, 32, 32, 512, 512),      # C5: two image rows per tile (4 x 34 pixels, three pieces), 32 slabs
    (1, 32, 32, 256, 256),      # P5
    (2, 16, 16, 64, 128),       # four rows per tile, pitch W + 16; a tile never straddles (256 % 64 == 0)
    (1, 33, 47, 192, 128),      # ragged rows: 5 x 49 pixels, pitch 63 (315 of the 320 slots), M % 64 != 0
    (3, 14, 14, 256, 256),      # tiles straddle images (two zero rows + the image skew inside the region)
    (1, 64, 64, 64, 320),       # four slabs only (the prologue's eleven fragment requests run past the end), ragged N
]


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", LAT_SHAPES)
def test_latency_form_of_the_halo_kernel_is_bit_identical(shape, dtype):
    """single-image grids run 64 x 64 tiles on four waves with deep prefetch (k_conv_halo_lat) — the same
    (slab, tap, part) order as the persistent 128 / 64-row kernel, hence the same bits; and repeatably (hand-counted vmcnt)."""
    B, H, W, Ci, Co = shape
    rng = np.random.default_rng(sum(shape) + 5)
    x = (rng.standard_normal((B, H, W, Ci)) * 2).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"halo_lat", 0))
        y0 = conv(x, w, 3, 1, scale, shift, None, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"halo_lat", 2))          # every grid under 3/4 of the chip (the policy, 1: under 3/8)
        ys = [conv(x, w, 3, 1, scale, shift, None, 1, dtype) for _ in range(3)]
        L.check(lib.mrcnn_debug_set(b"halo_lat", 1))
        ys.append(conv(x, w, 3, 1, scale, shift, None, 1, dtype))
    finally:
        L.check(lib.mrcnn_debug_set(b"halo_lat", 1))
    for y in ys:
        np.testing.assert_array_equal(y, y0)
    ref = torch_ref(x, w, 3, 1, scale, shift, None, 1, dtype)
    assert np.abs(y0 - ref).max() <= (4e-6 if dtype == "f32x3" else 2e-5) * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_round_aware_tile_height_is_bit_identical(dtype):
    """The mask head of a single image is 308 tiles of 128 x 128 — two rounds of the 256 persistent blocks, the second a fifth full: the launcher
    takes 64 x 128 tiles where their rounds come out shorter ("halo_rounds" 1).  A tile shape, not a summation order: same bits."""
    B, H, W, Ci, Co = 100, 14, 14, 256, 256
    rng = np.random.default_rng(123)
    x = (rng.standard_normal((B, H, W, Ci)) * 2).astype(np.float32)
    w = (rng.standard_normal((Co, 3, 3, Ci)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"halo_rounds", 0))
        y0 = conv(x, w, 3, 1, None, shift, None, 1, dtype)
    finally:
        L.check(lib.mrcnn_debug_set(b"halo_rounds", 1))
    y1 = conv(x, w, 3, 1, None, shift, None, 1, dtype)
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(conv(x[7:9], w, 3, 1, None, shift, None, 1, dtype), y1[7:9])


KCHUNK_SHAPES = [  # B, H, W, Cin, Cout, stride, residual — long-K 1x1 layers: 4 / 8 canonical chunks (conv_k_chunks)
    (1, 32, 32, 2048, 512, 1, False),      # C5 branch2a, single image: 8 M tiles -> four blocks per tile
    (2, 32, 32, 2048, 256, 1, True),       # the P5 lateral with a residual
    (1, 64, 64, 2048, 512, 2, False),      # stride-2 1x1
    (1, 31, 33, 2048, 300, 1, False),      # ragged M and N
    (600, 1, 1, 12544, 1024, 1, False),    # the box head's first inner product: eight chunks of 49 K steps
    (3, 7, 9, 2080, 64, 1, True),          # 65 K steps: the chunk count falls back to 1 (odd), 64-column tiles
    (2, 16, 16, 2112, 96, 1, False),       # 66 K steps: two chunks of 33, narrow tiles
    (1, 64, 64, 1024, 256, 1, False),      # K = 1024 stays one sum (C4 branch2a)
]


def _kchunk_operands(shape):
    B, H, W, Ci, Co, stride, with_res = shape
    rng = np.random.default_rng(sum(shape) + 41)
    x = rng.standard_normal((B, H, W, Ci), np.float32)
    w = (rng.standard_normal((Co, 1, 1, Ci), np.float32) * np.float32(1.0 / np.sqrt(Ci)))
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = rng.standard_normal(Co).astype(np.float32) * np.float32(0.1)
    oh, ow = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = rng.standard_normal((B, oh, ow, Co), np.float32) if with_res else None
    return x, w, scale, shift, res


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("shape", KCHUNK_SHAPES)
def test_shared_tiles_fold_the_k_chunks_in_the_canonical_order(shape, dtype):
    """the long-K 1x1 layers of the split modes sum ((0 + P0) + P1) + ... over canonical K chunks.  An
    under-filled grid gives every chunk its own block (partials through a scratch, the last block to arrive folds them); a
    full grid runs the chunks in one block.  Same bits either way, repeatably (the arrival order varies from launch to
    launch), and close to fp64."""
    x, w, scale, shift, res = _kchunk_operands(shape)
    stride = shape[5]
    lib = L.lib()
    try:
        L.check(lib.mrcnn_debug_set(b"conv_ksplit", 0))
        y0 = conv(x, w, 1, stride, scale, shift, res, 1, dtype)
        L.check(lib.mrcnn_debug_set(b"conv_ksplit", 1))
        L.check(lib.mrcnn_debug_set(b"conv_ksplit_below", 1 << 30))          # share whatever the grid
        ys = [conv(x, w, 1, stride, scale, shift, res, 1, dtype) for _ in range(4)]
        L.check(lib.mrcnn_debug_set(b"conv_min_blocks", 1))                   # ... and on the widest tiles
        ys.append(conv(x, w, 1, stride, scale, shift, res, 1, dtype))
    finally:
        L.check(lib.mrcnn_debug_set(b"conv_min_blocks", 448))
        L.check(lib.mrcnn_debug_set(b"conv_ksplit_below", 256))
        L.check(lib.mrcnn_debug_set(b"conv_ksplit", 1))
    for y in ys:
        np.testing.assert_array_equal(y, y0)
    ref = torch_ref(x, w, 1, stride, scale, shift, res, 1, dtype)
    assert np.abs(y0 - ref).max() <= (4e-6 if dtype == "f32x3" else 2e-5) * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_chunked_layers_do_not_depend_on_the_batch(dtype):
    """The sharding contract on the chunked layers: batch 8 fills the chip (one block per tile), a single image does not
    (a block per chunk) — the same bits per image."""
    rng = np.random.default_rng(77)
    for (B, H, Ci, Co) in [(8, 32, 2048, 512), (8, 32, 2048, 256), (24, 32, 2048, 512)]:
        x = rng.standard_normal((B, H, H, Ci), np.float32)
        w = (rng.standard_normal((Co, 1, 1, Ci), np.float32) * np.float32(1.0 / np.sqrt(Ci)))
        shift = (rng.standard_normal(Co) * 0.1).astype(np.float32)
        y = conv(x, w, 1, 1, None, shift, None, 1, dtype)
        for b in (0, B - 1):
            np.testing.assert_array_equal(conv(x[b:b + 1], w, 1, 1, None, shift, None, 1, dtype)[0], y[b], err_msg=f"{(B, H, Ci, Co)} image {b}")
        np.testing.assert_array_equal(conv(x[1:3], w, 1, 1, None, shift, None, 1, dtype), y[1:3])


ALIAS_SHAPES = [  # B, H, W, Cin, Cout, k — one per epilogue form a residual layer can take (the mode x tile class decides which)
    (2, 64, 64, 256, 1024, 1),     # C4 branch2c: 128-column tiles (split: wave-private fp32 epilogue; f16: wave_h; f32: wave)
    (1, 32, 32, 512, 2048, 1),     # C5 branch2c: narrowed N tile on an under-filled grid
    (2, 40, 40, 64, 256, 1),       # C2 branch2c: two K steps
    (1, 33, 47, 192, 300, 3),      # ragged everything: Cout 300 (Npad 384), M = 1551: the block-staged general epilogue
    (8, 64, 64, 256, 256, 3),      # 256-row ping-pong kernel in fp16 (direct epilogue, residual inside the store loop)
    (1, 32, 32, 2048, 256, 1),     # a chunked layer on an under-filled grid (split modes): the block that arrives last runs the epilogue of a shared tile
    (16, 32, 32, 2048, 256, 1),    # ... and on a full grid: one block folds the chunks (the four-wave 128-column form)
]


@pytest.mark.parametrize("dtype", ["f32", "f16", "f32s", "f32x3"])
@pytest.mark.parametrize("shape", ALIAS_SHAPES)
def test_every_epilogue_is_safe_in_place_over_its_residual(shape, dtype):
    """The engine writes every bottleneck block's output IN PLACE over its shortcut (engine_plan.hip: `to = sc`, res == out).  That
    rests on a contract of every epilogue form — a residual element is loaded by the thread that stores the output element at the
    same address, before the store (ConvDesc::res) — which nothing pinned: here each form runs with the output aliased
    onto the residual (mrcnn_debug_set("conv2d_alias_res", 1)) and must give the bits of the separate-buffer run, for every
    conv_direct policy (block-staged / direct / wave-private)."""
    B, H, W, Ci, Co, k = shape
    if dtype == "f16" and Ci % 64:
        pytest.skip("the fp16 kernels step K by 64 channels")
    rng = np.random.default_rng(sum(shape) + 31)
    x = rng.standard_normal((B, H, W, Ci), np.float32)
    w = (rng.standard_normal((Co, k, k, Ci), np.float32) * np.float32(1.0 / np.sqrt(k * k * Ci)))
    scale = (0.5 + rng.random(Co)).astype(np.float32)
    shift = rng.standard_normal(Co).astype(np.float32) * np.float32(0.1)
    res = rng.standard_normal((B, H, W, Co), np.float32)
    lib = L.lib()
    for direct in (0, 1, 2, 3):
        try:
            L.check(lib.mrcnn_debug_set(b"conv_direct", direct))
            y = conv(x, w, k, 1, scale, shift, res, 1, dtype)
            L.check(lib.mrcnn_debug_set(b"conv2d_alias_res", 1))
            y_inplace = conv(x, w, k, 1, scale, shift, res, 1, dtype)
        finally:
            L.check(lib.mrcnn_debug_set(b"conv2d_alias_res", 0))
            L.check(lib.mrcnn_debug_set(b"conv_direct", 3))
        np.testing.assert_array_equal(y_inplace, y, err_msg=f"conv_direct {direct}")
