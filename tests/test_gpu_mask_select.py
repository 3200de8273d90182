"""The mask head's row selection on caller data, in batches, with holes, in every tail form — through mrcnn_test_mask_select_batch
(include/maskrcnn_hip_test.h), which binds and strides the engine's routines as a predict does.  Whole-model predicts on random weights keep a
prefix of the rows, where compact index and row coincide: there a kernel reading det[mapping[i]] for det[i] passes.  (The one exception in the
suite: image 0 of the small model drops row 1, which tests/test_gpu_engine.py sees in three tests; a row the layer never writes it cannot see,
the engine clears the buffer first, nor the clamp, the padded strides, a lost write in every image of a batch, D > 128.)  The cases and THE definition (a plain numpy restatement of the rule) come from tests/mask_select_cases.py; their
conditions are proved in tests/test_mask_select_cases_host.py.  Per call:
  integers    flags, kept, the first kept[b] entries of mapping (the rest -1) and sel_cid: exact, per image.
  write set   out != sentinel equals the definition's write mask exactly, the [HW, out_stride) tails included; zeroed rows are bit-zero.
  form 2      values bit-identical to the selected class plane.
  form 1      against the float64 sigmoid of the float32 pre-activation the test forms itself (sequential sum of the parts, + bias: adds only).
              Bound 4 * 2^-24 absolute: no fast-math, so expf within 1 ulp, the add and the correctly rounded division within 0.5 ulp each, on a
              result of at most 1: about 2 ulp, with a factor 2 on top.
  form 0      against the float64 sigmoid of the float64 dot of the dtype-rounded feat with w.  Per element
              0.25 * (C * 2^-24 * sum |x_c w_c| + 2^-24 * |z|) + 4 * 2^-24: any summation order of C terms, sigmoid's slope at most 1/4, then
              the form-1 term.
  batch       image b alone gives the same bits as inside the batch.
Measured on an MI355X (every test prints its own figures):
  form 1: largest |got - ref| = 8.75e-8 = 1.47 * 2^-24 (bound 2.38e-7; 0.37 of it) over the seven calls.
  form 0: worst error / bound = 0.29 (C = 4, where the sigmoid term carries the bound); at C = 260 the ratio is 1.3e-3 .. 2.8e-3 — the bound
          allows every one of the C roundings its worst case with one sign, the kernel's 64-lane tree sum is far from it — still above 1e-3.
"""
import ctypes as C
import importlib
from dataclasses import replace

import numpy as np
import pytest

import conv_forms_cases as CK
import mask_select_cases as K
import test_gpu_conv_forms as CF

pytestmark = pytest.mark.gpu
F = np.float32
L = importlib.import_module("mask-rcnn-coreml_amd._lib")
DT = {"f32": L.F32, "f16": L.F16}
U = K.U24
SIGMOID_BOUND = 4 * U
ERR_INVALID, ERR_SHAPE = 1, 4


def descriptor(case, out, *, partial=None, pooled=None, row_len=0, keep):
    """The descriptor of a call and the arrays it points into (`keep` holds them alive and receives the optional outputs)."""
    o = case.ops
    arr = lambda k, a, t=F: keep.setdefault(k, np.ascontiguousarray(a, t))
    ptr = lambda k: keep[k].ctypes.data
    B, D, R = case.batch, case.d, case.det_rows
    q = L.MaskSelect(form=case.form, dtype=DT[case.dtype], batch=B, d=D, det_rows=R, hw=case.hw, nc=case.nc, det_stride=case.det.shape[2],
                     out_stride=out.shape[2])
    arr("det", case.det); q.det = ptr("det")
    q.out = out.ctypes.data
    if pooled is None:
        arr("flags", case.flags, np.int32); q.flags = ptr("flags")
    else:
        arr("pooled", pooled); q.pooled = ptr("pooled")
        q.row_len, q.row_stride, q.pooled_batch_stride = row_len, pooled.shape[2], pooled.shape[1] * pooled.shape[2]
    if case.form == 0:
        arr("feat", o["feat"]); arr("w", o["w"]); arr("bias", o["bias"])
        q.feat, q.w, q.bias, q.c = ptr("feat"), ptr("w"), ptr("bias"), o["feat"].shape[-1]
    elif case.form == 1:
        arr("partial", partial); arr("bias", o["bias"])
        assert keep["partial"].shape[:3] == (B, D, case.hw)
        q.partial, q.bias, q.parts = ptr("partial"), ptr("bias"), keep["partial"].shape[3]
    else:
        arr("masks", o["masks"]); q.masks = ptr("masks")
    for k, shape in (("row_flags", (B, D)), ("mapping", (B, D)), ("kept", (B,)), ("sel_cid", (B, R))):
        keep["got_" + k] = np.full(shape, -7, np.int32)
        setattr(q, k, keep["got_" + k].ctypes.data)
    return q


def run(case, partial=None, pooled=None, row_len=0):
    """One call on a sentinel-filled out -> {'out' (B, R, out_stride), 'flags', 'mapping', 'kept', 'sel_cid'}."""
    out = np.full((case.batch, case.det_rows, case.out_stride or case.hw), K.SENTINEL, F)
    keep = {}
    q = descriptor(case, out, partial=partial, pooled=pooled, row_len=row_len, keep=keep)
    L.check(L.lib().mrcnn_test_mask_select_batch(C.byref(q)))
    return {"out": out, "flags": keep["got_row_flags"], "mapping": keep["got_mapping"], "kept": keep["got_kept"], "sel_cid": keep["got_sel_cid"]}


def default_partial(case, exp):
    return K.partial_for(case, [e.sel_cid for e in exp]) if case.form == 1 else None


def check_integers_and_write_set(case, got, exp, label=""):
    for b, e in enumerate(exp):
        who = f"{case.name} {label} image {b}"
        np.testing.assert_array_equal(got["flags"][b], (case.flags[b] != 0).astype(np.int32), err_msg=who + ": flags")
        assert got["kept"][b] == e.kept, who
        np.testing.assert_array_equal(got["mapping"][b, :e.kept], e.mapping, err_msg=who + ": mapping")
        assert (got["mapping"][b, e.kept:] == -1).all(), who
        np.testing.assert_array_equal(got["sel_cid"][b], e.sel_cid, err_msg=who + ": sel_cid")
        o = got["out"][b]
        np.testing.assert_array_equal(o != K.SENTINEL, e.written, err_msg=who + ": write set")
        assert (o[e.kept:].view(np.uint32) == 0).all(), who + ": a padded row is not bit-zero"


def selected(exp, per_class):
    """per_class (B, D, nc, HW) -> (B, R, HW): the entry of each row's class, 0 where the row has none."""
    out = np.zeros((len(exp), len(exp[0].sel_cid), per_class.shape[-1]))
    for b, e in enumerate(exp):
        for r in np.flatnonzero(e.sel_cid >= 0):
            out[b, r] = per_class[b, r, e.sel_cid[r]]
    return out


def check_values(case, got, exp, z, mag, label=""):
    """-> the worst error / bound of the call (forms 0 and 1); form 2: bit identity."""
    hw = case.hw
    has = np.stack([e.sel_cid >= 0 for e in exp])                             # rows that carry a value
    want = np.stack([e.values[:, :hw] for e in exp])
    g = got["out"][..., :hw]
    if case.form == 2:
        np.testing.assert_array_equal(g[has], want[has].astype(F), err_msg=f"{case.name} {label}")
        return 0.0
    err = np.abs(g.astype(np.float64) - want)[has]
    if case.form == 1:
        bound = np.full(err.shape, SIGMOID_BOUND)
    else:
        bound = (0.25 * (case.ops["feat"].shape[-1] * U * selected(exp, mag) + U * np.abs(selected(exp, z))) + SIGMOID_BOUND)[has]
    ratio = float((err / bound).max())
    print(f"MASKSEL {case.name:48s} {label:12s} max err {err.max():.3e} worst err/bound {ratio:.4f}")
    assert (err <= bound).all(), (case.name, label, ratio)
    return ratio


def check_batch_independence(case, got, exp):
    partial = default_partial(case, exp)
    for b in range(case.batch):
        one = run(case.image(b), partial=None if partial is None else partial[b:b + 1])
        for k in got:
            np.testing.assert_array_equal(one[k][0], got[k][b], err_msg=f"{case.name}: {k} of image {b} alone")


def check_case(case):
    exp, z, mag = K.expect(case)
    got = run(case, partial=default_partial(case, exp))
    check_integers_and_write_set(case, got, exp)
    ratio = check_values(case, got, exp, z, mag)
    check_batch_independence(case, got, exp)
    return ratio


# ------------------------------------------------------------------------------------------------
# the three tails on the batch of six
# ------------------------------------------------------------------------------------------------
def _ids(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", K.FORM2, ids=_ids)
def test_full_form_copies_the_selected_plane(kw):
    check_case(K.make_case(2, **kw))


@pytest.mark.parametrize("kw", K.FORM1 + [None], ids=lambda kw: _ids(kw) if kw else "D130")
def test_fused_form_from_partials(kw):
    """Measured: see the module docstring (largest |got - ref| over these calls)."""
    check_case(K.make_case(1, **kw) if kw else K.wide_case())


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("kw", K.FORM0, ids=_ids)
def test_unfused_form_dot_and_sigmoid(kw, dtype):
    """Measured: see the module docstring (worst error / bound over these calls; above 1e-3, so the bound is not vacuous)."""
    assert check_case(K.make_case(0, dtype=dtype, **kw)) < 1.0


# ------------------------------------------------------------------------------------------------
# the predicate on pooled rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("row_len", K.ROW_LENS)
def test_predicate_on_pooled_rows(row_len, dtype):
    """k_mask_row_flags<float | _Float16> at row lengths around its 256-thread stride, the zero at either end and at index 256, -0.0, NaN, the
    fp16 subnormal, a value the fp16 rounding turns into zero; the gap behind a row is zero and must not be read; three images, three patterns."""
    rows, _ = K.pooled_rows(row_len)
    case = replace(K.predicate_case(row_len), dtype=dtype, flags=K.predicate_expect(row_len, dtype))
    exp, z, mag = K.expect(case)
    got = run(case, pooled=rows, row_len=row_len)
    check_integers_and_write_set(case, got, exp, dtype)
    check_values(case, got, exp, z, mag, dtype)
    for b in range(case.batch):
        one = run(case.image(b), pooled=rows[b:b + 1], row_len=row_len)
        for k in got:
            np.testing.assert_array_equal(one[k][0], got[k][b], err_msg=f"{case.name} {dtype}: {k} of image {b} alone")


# ------------------------------------------------------------------------------------------------
# the forms against each other
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [1, 2, 4])
def test_unfused_and_fused_forms_agree(parts):
    """Form 0 (fp32) and form 1 on the same rows: the partials are form 0's dot split into `parts` column groups on the host (float64 sums rounded
    to fp32).  Identical write sets; values within the sum of the two forms' bounds."""
    c0 = K.make_case(0, 197, c=260, out_extra=3, det_stride=7)
    exp, z, mag = K.expect(c0)
    x, w = c0.ops["feat"].astype(np.float64), c0.ops["w"].astype(np.float64)
    groups = np.array_split(np.arange(x.shape[-1]), parts)
    per_class = np.stack([np.einsum("bdpc,nc->bdnp", x[..., g], w[:, g]) for g in groups], -1).astype(F)
    c1 = replace(c0, form=1, name=f"form1-of-form0-parts{parts}", ops={"per_class": per_class, "bias": c0.ops["bias"]})
    exp1, z1, _ = K.expect(c1)
    g0 = run(c0)
    g1 = run(c1, partial=default_partial(c1, exp1))
    check_integers_and_write_set(c0, g0, exp)
    check_integers_and_write_set(c1, g1, exp1)
    np.testing.assert_array_equal(g0["out"] != K.SENTINEL, g1["out"] != K.SENTINEL)
    has = np.stack([e.sel_cid >= 0 for e in exp])
    bound = (0.25 * (260 * U * selected(exp, mag) + U * np.abs(selected(exp, z))) + 2 * SIGMOID_BOUND)[has]
    diff = np.abs(g0["out"][..., :197].astype(np.float64) - g1["out"][..., :197])[has]
    print(f"MASKSEL forms 0 / 1 parts {parts}: max diff {diff.max():.3e} worst diff/bound {(diff / bound).max():.4f}")
    assert (diff <= bound).all()


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_fused_tail_end_to_end_equals_the_unfused_tail(mode):
    """conv_forms_cases' selected_128 shape (5 rows, 7 x 7 -> 14 x 14, Cout 128): sel_cid from this entry for a hole pattern goes to the
    deconvolution's selected-class epilogue, its partials come back into form 1; form 0 runs on the stored deconvolution output of the same
    operands.  Same write set; values within conv_forms_cases' bound of the selected dot through the sigmoid's slope of 1/4 — under both
    "mask_sel_wave" settings (64- and 128-column partial sums: parts 2 and 1)."""
    f = CK.SEL_FORMS[0]
    assert (f.name, f.B, f.Cout) == ("selected_128", 5, 128)
    hw = 4 * f.H * f.W
    flags = np.array([[1, 0, 1, 1, 0]], np.int32)                    # nk = 3, mapping 0,2,3: row 2 <- detection 1's class, the write to row 3 lost
    det = np.zeros((1, 5, 6), F)
    det[0, :, 4] = (3, 1, 0, 4, 2)
    det[0, :, 5] = 0.9
    ops = CK.make_operands(f)
    bias = (0.25 * np.arange(f.nc) - 0.5).astype(F)
    plain = replace(f, nc=0, sel_cid=())
    stored = CF.run(plain, mode, {k: v for k, v in ops.items() if k != "sel_w"})["out"].reshape(1, 5, hw, f.Cout)
    c0 = K.Case("end-to-end-form0", 0, flags, det, hw, f.nc, mode, 0, {"feat": stored, "w": ops["sel_w"], "bias": bias})
    exp = K.expect(c0)[0]
    g0 = run(c0)
    check_integers_and_write_set(c0, g0, exp)
    sel = g0["sel_cid"][0]
    assert list(sel) == [3, -1, 1, -1, -1]
    fs = replace(f, sel_cid=tuple(int(v) for v in sel))
    ref = CK.reference(fs, mode, ops)
    bound = 0.25 * CK.selected_bound(fs, mode, ref["abs"])
    for wave, parts in ((1, 2), (0, 1)):
        with CF.knobs(mask_sel_wave=wave):
            partial = CF.run(fs, mode, ops)["partial"]
        assert partial.shape == (5, hw, parts)
        c1 = K.Case(f"end-to-end-form1-wave{wave}", 1, flags, det, hw, f.nc, "f32", 0, {"bias": bias})
        g1 = run(c1, partial=partial[None])
        for k in ("flags", "mapping", "kept", "sel_cid"):
            np.testing.assert_array_equal(g1[k], g0[k])
        np.testing.assert_array_equal(g1["out"] != K.SENTINEL, g0["out"] != K.SENTINEL)
        rows = np.flatnonzero(sel >= 0)
        diff = np.abs(g1["out"][0, rows].astype(np.float64) - g0["out"][0, rows])
        print(f"MASKSEL end to end {mode} mask_sel_wave {wave}: max diff {diff.max():.3e} worst diff/bound {(diff / bound[rows]).max():.4f}")
        assert (diff <= bound[rows]).all()
        # and each against the float64 definition of the whole tail: sigmoid(dot + bias)
        want = K.sigmoid(ref["dot"][rows] + bias[sel[rows]].astype(np.float64)[:, None])
        assert (np.abs(g1["out"][0, rows] - want) <= bound[rows] + SIGMOID_BOUND).all()


# ------------------------------------------------------------------------------------------------
# the stand-alone layer: more detections than feature rows
# ------------------------------------------------------------------------------------------------
def test_mask_layer_pads_up_to_the_detection_count(pkg, orc, small_model):
    """TimeDistributedMaskLayer.evaluate with 14 detection rows over 12 feature rows: the predicate runs on the 12, the zero padding on to row
    14 (tests/test_gpu_layers.py::test_mask_layer has the two counts equal).  Against the oracle model; 2e-4 absolute on sigmoid outputs, as there."""
    import os
    from oracle.network import load_oracle_model
    d, cfg = small_model
    om = load_oracle_model(d)
    pkg.MaskRCNNConfig.defaultConfig().compiledMaskModelURL = os.path.join(d, "Mask.mrcw")
    rng = np.random.default_rng(14)
    D, R = 12, 14
    pooled = rng.standard_normal((D, 1, 256, 14, 14)).astype(F)
    pooled[1] = 0
    pooled[5, 0, 7, 3, 2] = 0
    pooled[8:11] = 0                                            # kept: 0,2,3,4,6,7,11 -> nk = 7; the write to row 11 is lost
    det = np.zeros((R, 6), F)
    det[:, 4] = 1 + (3 * np.arange(R)) % (cfg.num_classes - 1)
    det[:, 5] = 0.9
    out = np.full((1, 1, R, 28, 28), F(5.0))
    layer = pkg.TimeDistributedMaskLayer({})
    layer.evaluate([pkg.MLMultiArray(pooled), pkg.MLMultiArray(det)], [pkg.MLMultiArray(out)])
    want = om.masks(pooled.reshape(D, 256, 14, 14), det, out=np.full((R, 784), F(5.0)))
    got = out.reshape(R, 784)
    np.testing.assert_array_equal(got == 5.0, want == 5.0)
    assert (got[7:] == 0).all() and (got[[1, 5]] == 5.0).all() and (got[0] != 5.0).all()
    np.testing.assert_allclose(got[want != 5.0], want[want != 5.0], atol=2e-4)


# ------------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------------
def test_bad_arguments_return_a_status_and_leave_out_untouched():
    lib = L.lib()
    cases = {0: K.make_case(0, 3, c=8), 1: K.make_case(1, 3, parts=2), 2: K.make_case(2, 3)}
    rows, _ = K.pooled_rows(255)

    def refused(which, status, from_rows=None, **change):
        case = cases[which] if from_rows is None else K.predicate_case(255)
        exp = K.expect(case)[0]
        out = np.full((case.batch, case.det_rows, case.hw), K.SENTINEL, F)
        keep = {}
        q = descriptor(case, out, partial=default_partial(case, exp), pooled=from_rows, row_len=255 if from_rows is not None else 0, keep=keep)
        for k, v in change.items():
            setattr(q, k, v)
        st = lib.mrcnn_test_mask_select_batch(C.byref(q))
        assert st == status, (which, change, st, lib.mrcnn_last_error())
        assert lib.mrcnn_last_error(), change
        assert (out == K.SENTINEL).all(), change

    assert lib.mrcnn_test_mask_select_batch(None) == ERR_INVALID
    for which in (0, 1, 2):
        refused(which, ERR_INVALID, det=None)
        refused(which, ERR_INVALID, flags=None)                                   # neither predicate source
        refused(which, ERR_INVALID, pooled=rows.ctypes.data, row_len=255, row_stride=260, pooled_batch_stride=8 * 260)        # both
        refused(which, ERR_INVALID, form=3)
        refused(which, ERR_INVALID, form=-1)
        refused(which, ERR_INVALID, det_rows=K.D - 1)
        refused(which, ERR_INVALID, det_stride=5)
        refused(which, ERR_INVALID, out_stride=2)
        refused(which, ERR_INVALID, dtype=L.F32S)
        for k in ("batch", "d", "hw", "nc"):
            refused(which, ERR_INVALID, **{k: 0})
    for k in ("feat", "w", "bias"):
        refused(0, ERR_INVALID, **{k: None})
    refused(0, ERR_SHAPE, c=6)
    refused(0, ERR_SHAPE, c=0)
    for k in ("partial", "bias"):
        refused(1, ERR_INVALID, **{k: None})
    refused(1, ERR_INVALID, parts=0)
    refused(2, ERR_INVALID, masks=None)
    refused(2, ERR_INVALID, from_rows=rows, row_stride=254)                         # under row_len
    refused(2, ERR_INVALID, from_rows=rows, pooled_batch_stride=8 * 260 - 1)        # under d rows
    refused(2, ERR_INVALID, from_rows=rows, row_len=0)
    refused(2, ERR_INVALID, out=None)
