"""The convolution forms only the engine builds, one conv_forward at a time through mrcnn_test_conv_form_nhwc (include/maskrcnn_hip_test.h).

mrcnn_conv2d_nhwc describes a dense layer; the engine also runs the FPN laterals' shifted residual (res_shift), the unfused RPN heads'
column split into two pitched buffers (out2 / n_split), the P6 view's strided input, the mask head's 2 x 2 scatter (deconv2), its
selected-class dot (sel_partial) and fp32 stores of fp16 tensors (out_f32) — until now checked only through whole predicts, at the
geometries a predict happens to produce.  Here each form runs alone, in all four compute modes, at levels that are odd, not a power
of two, with image boundaries and class changes inside a 128-row tile, and for every case:

  1. float64       the definition of tests/conv_forms_cases.py (pinned on the CPU by tests/test_conv_forms_host.py), at the per-mode
                   tolerances of tests/test_gpu_conv_kernels.py; the selected-class partial sums, summed over their parts, inside
                   the derived forward error Cout * 2^-24 * sum |y w| (+ 2^-11 * sum |y w| in f16, where y is rounded first)
  2. write set     every buffer is sentinel-filled by the entry and comes back whole: outside the addressed elements (pitch gaps,
                   between images, in front, behind, the partial sums of -1 rows) the sentinel stands, inside it does not
  3. bit identity  across the dispatcher's choices that are documented to change no bit ("conv_direct" 0..3, the N tile through
                   "conv_min_blocks", "conv_tn4", the ping-pong kernel where a case qualifies); "conv_halo" and "mask_sel_wave"
                   differ by summation noise, so each side meets float64 on its own
  4. batch         image (ROI row) b of the batch equals the same image run alone, bit for bit

and one watchdog test per form (mrcnn_test_last_range_flag, in the style of tests/test_gpu_range_watch.py).

Worst |got - ref| per form as measured on an MI355X (every test prints its own; the bound is tol * max(1, |ref|.max()), about 1.0e-2 .. 1.5e-2
in f16, 1e-4 in f32 / f32s, 5e-5 in f32x3):

  form                   f16       f32       f32s      f32x3
  lateral_odd_level      1.95e-3   1.66e-6   1.45e-6   1.45e-6
  lateral_24x24          1.95e-3   3.19e-6   1.40e-6   1.40e-6
  lateral_36_columns     1.93e-3   1.51e-6   6.26e-7   6.54e-7
  lateral_30_columns     1.88e-3   1.20e-6   5.77e-7   6.34e-7
  lateral_3x3            1.95e-3   5.24e-6   2.41e-6   2.41e-6
  lateral_relu           1.95e-3   1.81e-6   8.73e-7   8.73e-7
  rpn_heads_cin64        5.15e-7   8.63e-7   6.87e-7   6.87e-7      (f16 stores fp32 here: out_f32)
  rpn_heads_cin512       1.05e-6   3.30e-6   1.25e-6   1.25e-6
  p6_view_3x3            9.75e-4   2.73e-6   1.82e-6   1.82e-6
  deconv_128             1.94e-3   1.66e-6   8.02e-7   8.02e-7
  deconv_32              1.94e-3   1.47e-6   8.79e-7   8.79e-7
  deconv_20              1.83e-3   1.57e-6   7.96e-7   7.96e-7
  deconv_32_row_pitch    1.84e-3   1.17e-6   1.02e-6   1.02e-6
  selected_128 (err / its bound Cout * 2^-24 * sum |y w| [+ 2^-11 * sum |y w|])   0.28   0.018   0.013   0.011
  selected_256                                                                    0.18   0.007   0.005   0.005
"""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import conv_forms_cases as K

pytestmark = pytest.mark.gpu
L = importlib.import_module("mask-rcnn-coreml_amd._lib")

DT = {"f32": L.F32, "f16": L.F16, "f32s": L.F32S, "f32x3": L.F32X3}
SPLIT = ("f32s", "f32x3")
WATCHED = ("f16", "f32s", "f32x3")          # the exact-fp32 mode has no fp16 hand-over: its word stays 0

# the shipped value of every knob these tests touch (restored in `finally`, in this order: "conv_min_blocks" sets both thresholds)
DEFAULTS = {"conv_halo": 1, "conv_pp": 1, "conv_pp_min_tiles": 512, "conv_pp_min_kt": 16, "conv_pp_min_fill": 85, "conv_pp_split": 0, "conv_tn4": -1,
            "conv_direct": 3, "conv_min_blocks": 448, "conv_min_blocks_split": 256, "mask_sel_wave": 1}
PINGPONG = {"conv_pp": 1, "conv_pp_min_tiles": 1, "conv_pp_min_kt": 2, "conv_pp_min_fill": 0, "conv_pp_split": 1}       # as test_pingpong_kernel_equals_128row_kernel_bitwise
# Choices that change no bit (include/maskrcnn_hip_test.h), each compared with the shipped policy.  On grids this small the policy narrows
# the N tile to 32 columns, whose only epilogue is the block-staged one: the wave-private and straight-from-the-accumulators forms are
# reached with the widest tile ("conv_min_blocks" 1) under each "conv_direct".
SAME_BITS = [{"conv_direct": 0}, {"conv_direct": 1}, {"conv_direct": 2}, {"conv_min_blocks": 1}, {"conv_min_blocks": 1 << 30},
             {"conv_direct": 1, "conv_min_blocks": 1}, {"conv_direct": 2, "conv_min_blocks": 1},
             {"conv_tn4": 0}, {"conv_tn4": 1}, {"conv_tn4": 1, "conv_direct": 0, "conv_min_blocks": 1}, {"conv_tn4": 1, "conv_min_blocks": 1}]


@contextlib.contextmanager
def knobs(**kv):
    try:
        for k, v in kv.items():
            assert k in DEFAULTS, k
            L.check(L.lib().mrcnn_debug_set(k.encode(), int(v)))
        yield
    finally:
        for k in DEFAULTS:
            if k in kv or (k == "conv_min_blocks_split" and "conv_min_blocks" in kv):
                L.check(L.lib().mrcnn_debug_set(k.encode(), DEFAULTS[k]))


def run(f, mode, ops):
    """One launch -> {'out' / 'out2': the whole float32 buffers, 'partial': (B, 4HW, parts), 'flag': the watchdog word}."""
    keep = {k: np.ascontiguousarray(v, np.float32) for k, v in ops.items()}
    ptr = lambda k: keep[k].ctypes.data if k in keep else None
    form = L.ConvForm(dtype=DT[mode], batch=f.B, h=f.H, w=f.W, cin=f.Cin, cout=f.Cout, ksize=f.k, stride=f.stride, act=f.act, in_step=f.in_step,
                      res_shift=max(f.res_shift, 0), n_split=f.n_split, deconv2=int(f.deconv2), out_f32=int(f.out_f32 and mode == "f16"), nc=f.nc,
                      sentinel=K.SENTINEL, in_=ptr("x"), filters=ptr("w"), scale=ptr("scale"), shift=ptr("shift"), residual=ptr("res"), sel_w=ptr("sel_w"))
    got = {}
    if f.nc:
        cid = np.asarray(f.sel_cid, np.int32)
        assert cid.shape == (f.B,)
        partial = np.full((f.B, 4 * f.H * f.W, f.Cout // 64), np.nan, np.float32)          # sized for the most parts
        parts = C.c_int32(0)
        form.sel_cid, form.sel_partial, form.sel_parts = cid.ctypes.data, partial.ctypes.data, C.addressof(parts)
    else:
        for which in ("out", "out2") if f.n_split else ("out",):
            lo = K.layout_of(f, which)
            got[which] = np.full(lo["len"], np.nan, np.float32)
            setattr(form, which, L.ConvFormOutput(data=got[which].ctypes.data, len=lo["len"], offset=lo["offset"], batch_stride=lo["batch_stride"],
                                                  pitch=lo["pitch"], row_pitch=lo["row_pitch"] if f.deconv2 else 0))
    L.check(L.lib().mrcnn_test_conv_form_nhwc(C.byref(form)))
    if f.nc:
        assert parts.value in (f.Cout // 64, f.Cout // 128)
        got["partial"] = partial.reshape(-1)[:f.B * 4 * f.H * f.W * parts.value].reshape(f.B, 4 * f.H * f.W, parts.value).copy()
    flag = C.c_int(-1)
    L.check(L.lib().mrcnn_test_last_range_flag(C.byref(flag)))
    got["flag"] = flag.value
    return got


def same_bits(a, b, what):
    for k in a:
        if k != "flag":
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    assert a["flag"] == b["flag"], what


def check_float64_and_write_set(f, mode, got, ref, label=""):
    """Assertions 1 and 2 of a plain (stored) form."""
    errs, mags = [], []
    for which, (buf, mask) in ref.items():
        g = got[which].astype(np.float64)
        assert g.shape == buf.shape
        stray = np.flatnonzero(~mask & (g != K.SENTINEL))
        assert stray.size == 0, f"{f.name} {mode} {label}: {which} written outside the addressed elements, first at {stray[:8]} of {g.size}"
        missed = np.flatnonzero(mask & ~(g != K.SENTINEL))
        assert missed.size == 0, f"{f.name} {mode} {label}: {which} not written at {missed[:8]}"
        errs.append(np.abs(g[mask] - buf[mask]).max())
        mags.append(np.abs(buf[mask]).max())
    err, bound = max(errs), K.TOL[mode] * max(1.0, max(mags))
    print(f"CONVFORM {f.name:24s} {mode:6s} {label:16s} err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (f.name, mode, label, err, bound)


def check_selected(f, mode, got, ref, label=""):
    """Assertions 1 and 2 of the selected-class form: the parts of a pixel sum to the float64 dot; -1 rows keep the sentinel."""
    p = got["partial"].astype(np.float64)
    wr = ref["written"]
    assert (p[~wr] == K.SENTINEL).all(), f"{f.name} {mode} {label}: partial sums of a -1 row were written"
    assert (p[wr] != K.SENTINEL).all() and np.isfinite(p[wr]).all(), f"{f.name} {mode} {label}: partial sums of a written row are missing"
    err = np.abs(p.sum(-1) - ref["dot"])[wr]
    bound = K.selected_bound(f, mode, ref["abs"])[wr]
    worst = np.argmax(err / bound)
    print(f"CONVFORM {f.name:24s} {mode:6s} {label:16s} err {err.max():.3e} bound(at worst ratio) {bound.reshape(-1)[worst]:.3e} "
          f"worst err/bound {(err / bound).max():.3f} parts {p.shape[-1]}")
    assert (err <= bound).all(), (f.name, mode, label, float((err / bound).max()))


def check_batch_independence(f, mode, ops, got):
    for b in range(f.B):
        one = run(f.image(b), mode, K.image_operands(ops, b))
        if f.nc:
            np.testing.assert_array_equal(one["partial"][0], got["partial"][b], err_msg=f"{f.name} {mode}: ROI row {b}")
            continue
        for which in got:
            if which == "flag":
                continue
            a1 = K.addresses(K.layout_of(f.image(b), which), 1)
            ab = K.addresses(K.layout_of(f, which), f.B)[b:b + 1]
            np.testing.assert_array_equal(one[which][a1], got[which][ab], err_msg=f"{f.name} {mode}: {which} of image {b}")


def cases(forms, modes=K.MODES):
    return [pytest.param(f, m, id=f"{f.name}-{m}") for f in forms for m in modes]


# ---------------------------------------------------------------------------------------------------------------------
# the stored forms: shifted residual, column split, 2 x 2 scatter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,mode", cases(K.RES_SHIFT_FORMS + K.SPLIT_FORMS + K.DECONV_FORMS))
def test_stored_form_against_float64_write_set_dispatch_and_batch(f, mode):
    ops = K.make_operands(f)
    ref = K.reference(f, mode, ops)
    got = run(f, mode, ops)
    assert got["flag"] == 0
    check_float64_and_write_set(f, mode, got, ref)
    for kv in SAME_BITS:
        if "conv_tn4" in kv and mode not in SPLIT:
            continue
        with knobs(**kv):
            same_bits(run(f, mode, ops), got, f"{f.name} {mode} {kv}")
    check_batch_independence(f, mode, ops, got)


@pytest.mark.parametrize("mode", WATCHED)          # (the ping-pong kernel has no exact-fp32 form)
def test_shifted_residual_on_the_pingpong_kernel_equals_the_128row_kernel_bitwise(mode):
    f = next(f for f in K.RES_SHIFT_FORMS if f.name == "lateral_24x24")
    ops = K.make_operands(f)
    with knobs(conv_pp=0):
        y0 = run(f, mode, ops)
    with knobs(**PINGPONG):
        y1 = run(f, mode, ops)
    same_bits(y1, y0, f"{f.name} {mode} ping-pong")
    check_float64_and_write_set(f, mode, y1, K.reference(f, mode, ops), "ping-pong")


# ---------------------------------------------------------------------------------------------------------------------
# the strided input view: the halo kernel and the 128-row kernel have their own K orders — each against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,mode", cases(K.STRIDED_FORMS))
def test_strided_input_against_float64_write_set_dispatch_and_batch(f, mode):
    ops = K.make_operands(f)
    ref = K.reference(f, mode, ops)
    for halo in (1, 0) if mode in SPLIT else (1,):
        with knobs(conv_halo=halo):
            got = run(f, mode, ops)
            assert got["flag"] == 0
            check_float64_and_write_set(f, mode, got, ref, f"conv_halo {halo}")
            for kv in SAME_BITS:
                if "conv_tn4" in kv and mode not in SPLIT:
                    continue
                with knobs(**kv):
                    same_bits(run(f, mode, ops), got, f"{f.name} {mode} conv_halo {halo} {kv}")
            check_batch_independence(f, mode, ops, got)


# ---------------------------------------------------------------------------------------------------------------------
# the selected-class dot: 64- and 128-column partial sums differ by summation noise — each against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f,mode", cases(K.SEL_FORMS))
def test_selected_class_against_float64_write_set_dispatch_and_batch(f, mode):
    ops = K.make_operands(f)
    ref = K.reference(f, mode, ops)
    for wave in (1, 0):
        with knobs(mask_sel_wave=wave):
            got = run(f, mode, ops)
            assert got["flag"] == 0
            assert got["partial"].shape[-1] == f.Cout // (64 if wave else 128)
            check_selected(f, mode, got, ref, f"mask_sel_wave {wave}")
            for kv in SAME_BITS:
                if "conv_tn4" in kv and mode not in SPLIT:
                    continue
                with knobs(**kv):
                    same_bits(run(f, mode, ops), got, f"{f.name} {mode} mask_sel_wave {wave} {kv}")
            check_batch_independence(f, mode, ops, got)


# ---------------------------------------------------------------------------------------------------------------------
# what the dispatcher cannot run is refused with a message
# ---------------------------------------------------------------------------------------------------------------------
def test_unsupported_combinations_are_refused_loudly():
    base = K.DECONV_FORMS[1]
    bad = [
        (K.replace(K.SEL_FORMS[0], Cout=96), "partial sums"),                                         # the selected-class mode works in 64- / 128-column parts
        (K.replace(base, k=3), "deconv2"),                                                            # the scatter is a 1x1 GEMM
        (K.replace(base, res_shift=0), "deconv2"),                                                    # ... without a residual
        (K.replace(K.RES_SHIFT_FORMS[0], Cin=48), "Cin"),                                             # K tile
        (K.replace(K.SPLIT_FORMS[0], n_split=18), "n_split"),
    ]
    for f, word in bad:
        ops = K.make_operands(f)
        with pytest.raises(L.MrcnnError) as e:
            run(f, "f32s", ops)
        assert word in str(e.value), (f.name, str(e.value))
    # an output whose images would not fit its buffer is refused before anything is launched
    f = K.SPLIT_FORMS[0]
    ops = K.make_operands(f)
    keep = {k: np.ascontiguousarray(v, np.float32) for k, v in ops.items()}
    lo, lo2 = K.layout_of(f, "out"), K.layout_of(f, "out2")
    o1, o2 = np.zeros(lo["len"], np.float32), np.zeros(lo2["len"], np.float32)
    form = L.ConvForm(dtype=L.F32S, batch=f.B, h=f.H, w=f.W, cin=f.Cin, cout=f.Cout, ksize=1, stride=1, in_step=1, n_split=f.n_split, sentinel=K.SENTINEL,
                      in_=keep["x"].ctypes.data, filters=keep["w"].ctypes.data,
                      out=L.ConvFormOutput(data=o1.ctypes.data, len=lo["len"] - f.out.gap - f.out.tail - 1, offset=lo["offset"], batch_stride=lo["batch_stride"], pitch=lo["pitch"]),
                      out2=L.ConvFormOutput(data=o2.ctypes.data, len=lo2["len"], offset=lo2["offset"], batch_stride=lo2["batch_stride"], pitch=lo2["pitch"]))
    with pytest.raises(L.MrcnnError) as e:
        L.check(L.lib().mrcnn_test_conv_form_nhwc(C.byref(form)))
    assert "do not fit" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# the fp16-range watchdog, one test per form: ONE stored value beyond 65504 sets bit 0, the same operands halved do not
# ---------------------------------------------------------------------------------------------------------------------
BIG = 60000.0          # an fp16 value (a multiple of 32); times a scale of 2: 120000 >= 65504, halved: 60000 < 65504


def quiet_operands(f, seed=1):
    """Random operands with input channel 0 spare — zero in the activations and in every filter — for the plants; unit scale, no shift."""
    ops = K.make_operands(f, seed)
    ops["x"] *= np.float32(0.25)
    ops["x"][..., 0] = 0
    ops["w"][..., 0] = 0
    ops["scale"] = np.ones(f.Cout, np.float32)
    ops["shift"] = np.zeros(f.Cout, np.float32)
    return ops


@pytest.mark.parametrize("mode", WATCHED)
def test_watchdog_sees_a_value_that_leaves_the_range_only_through_the_shifted_residual(mode):
    """Level 5 x 7 under a 3 x 4 upper level: the upper pixel (2, 3) feeds the output pixel (4, 6) alone.  Channel c carries 30000 everywhere (the
    shift) and 40000 more at that one upper pixel: 70000 at ONE stored element, and at none when either half is missing or both are halved."""
    f = K.Form("watch_lateral", 2, 5, 7, 64, 32, res_shift=1)
    c, b = 21, 1
    for direct in (0, 3):
        ops = quiet_operands(f)
        ops["res"] *= np.float32(0.25)
        ops["shift"][c] = 30000.0
        with knobs(conv_direct=direct):
            assert run(f, mode, ops)["flag"] == 0                      # the shift alone
            ops["res"][b, 2, 3, c] = 40000.0
            got = run(f, mode, ops)
            assert got["flag"] == 1, (mode, direct)
            y = got["out"][K.addresses(K.layout_of(f, "out"), f.B)].astype(np.float64)
            over = np.argwhere(~(np.abs(y) < 65504.0))
            np.testing.assert_array_equal(over, [[b, 4, 6, c]])
            half = dict(ops, res=ops["res"] * np.float32(0.5), shift=ops["shift"] * np.float32(0.5), x=ops["x"] * np.float32(0.5))
            assert run(f, mode, half)["flag"] == 0
            ops["shift"][c] = 0.0                                      # the residual alone
            assert run(f, mode, ops)["flag"] == 0


@pytest.mark.parametrize("mode", WATCHED)
def test_watchdog_sees_a_value_in_an_out2_column(mode):
    f = K.replace(K.SPLIT_FORMS[0], name="watch_rpn_heads")
    b, oh, ow = 1, 2, 3
    for n in (f.n_split + 5, f.Cout - 1, 2):                          # two columns of out2, one of out
        ops = quiet_operands(f)
        assert run(f, mode, ops)["flag"] == 0                          # (the padded columns 18..31 carry a shift of 1e30: never stored, never watched)
        ops["x"][b, oh, ow, 0] = 1.0
        ops["w"][n, 0, 0, 0] = BIG
        ops["scale"][n] = 2.0
        got = run(f, mode, ops)
        assert got["flag"] == 1, (mode, n)
        which, col = ("out2", n - f.n_split) if n >= f.n_split else ("out", n)
        for k in ("out", "out2"):
            y = got[k][K.addresses(K.layout_of(f, k), f.B)].astype(np.float64)
            over = np.argwhere(~(np.abs(y) < 65504.0))
            np.testing.assert_array_equal(over, [[b, oh, ow, col]] if k == which else np.empty((0, 4), int))
        assert run(f, mode, dict(ops, x=ops["x"] * np.float32(0.5)))["flag"] == 0


@pytest.mark.parametrize("mode", WATCHED)
def test_watchdog_sees_a_value_in_each_deconv2_quadrant(mode):
    for f in (K.replace(K.DECONV_FORMS[1], name="watch_deconv_32"), K.replace(K.DECONV_FORMS[2], name="watch_deconv_20")):      # vector / (f16) scalar; 80 columns padded to 128
        b, h, w, co = f.B - 1, f.H - 1, 2, f.Cout - 3
        for dy in range(2):
            for dx in range(2):
                ops = quiet_operands(f)
                if dy == dx == 0:
                    assert run(f, mode, ops)["flag"] == 0
                ops["x"][b, h, w, 0] = 1.0
                ops["w"][dy, dx, co, 0] = BIG
                ops["scale"][co] = 2.0
                got = run(f, mode, ops)
                assert got["flag"] == 1, (f.name, mode, dy, dx)
                y = got["out"][K.addresses(K.layout_of(f, "out"), f.B)].astype(np.float64)
                np.testing.assert_array_equal(np.argwhere(~(np.abs(y) < 65504.0)), [[b, 2 * h + dy, 2 * w + dx, co]])
                assert run(f, mode, dict(ops, x=ops["x"] * np.float32(0.5)))["flag"] == 0


@pytest.mark.parametrize("wave", [1, 0])
@pytest.mark.parametrize("mode", WATCHED)
def test_watchdog_sees_the_activated_value_inside_the_selected_class_epilogue(mode, wave):
    """Nothing is stored but the dots: the watched value is the activated y the dot reads.  A row with class -1 is not written and has no
    output to watch: the same plant there leaves the word 0."""
    f = K.replace(K.SEL_FORMS[0], name="watch_selected")
    h, w, dy, dx, co = 3, 5, 1, 0, 77
    with knobs(mask_sel_wave=wave):
        for b, want in ((3, 1), (0, 1), (1, 0)):                       # rows of classes 4, 3 and -1
            assert (f.sel_cid[b] >= 0) == bool(want)
            ops = quiet_operands(f)
            if b == 3:
                assert run(f, mode, ops)["flag"] == 0
            ops["x"][b, h, w, 0] = 1.0
            ops["w"][dy, dx, co, 0] = BIG
            ops["scale"][co] = 2.0
            got = run(f, mode, ops)
            assert got["flag"] == want, (mode, wave, b)
            assert (got["partial"][1] == K.SENTINEL).all()
            assert run(f, mode, dict(ops, x=ops["x"] * np.float32(0.5)))["flag"] == 0
            ops["w"][dy, dx, co, 0] = -BIG                             # cleared by the ReLU before the dot reads it
            assert run(f, mode, ops)["flag"] == 0
