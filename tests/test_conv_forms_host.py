"""The float64 definitions of tests/conv_forms_cases.py, each against an independent statement of the same operation, on the CPU.

tests/test_gpu_conv_forms.py holds the kernels to those definitions; a mistake in one of them would either fail the kernels
wrongly or, worse, agree with a kernel that shares it.  Here every definition (written as index arithmetic) meets a library
operation that says the same thing another way, on small random float64 data: agreement to float64 rounding.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_forms_cases as K


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@pytest.mark.parametrize("oh,ow", [(13, 10), (24, 24), (6, 6), (9, 7), (1, 1), (2, 5)])
def test_shifted_residual_is_the_upper_level_repeated_and_cropped(oh, ow):
    rng = np.random.default_rng(oh * 31 + ow)
    res = rng.standard_normal((3, (oh + 1) // 2, (ow + 1) // 2, 5))
    want = _t(res).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :oh, :ow].numpy()
    np.testing.assert_array_equal(K.ref_shifted_residual(res, oh, ow, 1), want)
    np.testing.assert_array_equal(K.ref_shifted_residual(want, oh, ow, 0), want)          # shift 0: the residual itself


@pytest.mark.parametrize("k,stride,in_step,h,w", [(3, 1, 2, 5, 7), (3, 1, 1, 6, 5), (1, 1, 2, 4, 3), (3, 2, 1, 9, 7), (1, 2, 1, 5, 6), (3, 2, 2, 5, 4)])
def test_strided_input_is_a_slice_followed_by_an_ordinary_convolution(k, stride, in_step, h, w):
    rng = np.random.default_rng(k * 100 + stride * 10 + in_step + h)
    x = rng.standard_normal((2, h * in_step, w * in_step, 6))
    wt = rng.standard_normal((4, k, k, 6))
    view = x[:, ::in_step, ::in_step]
    assert view.shape[1:3] == (h, w)
    want = F.conv2d(_t(view).permute(0, 3, 1, 2), _t(wt).permute(0, 3, 1, 2), stride=stride, padding=k // 2).permute(0, 2, 3, 1).numpy()
    got = K.ref_conv_strided(x, wt, k, stride, in_step)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("h,w,ci,co", [(7, 7, 6, 8), (5, 7, 3, 5), (1, 1, 4, 2)])
def test_deconv2_is_conv_transpose2d_with_stride_2(h, w, ci, co):
    rng = np.random.default_rng(h * 7 + w + ci + co)
    x = rng.standard_normal((3, h, w, ci))
    wt = rng.standard_normal((2, 2, co, ci))                       # (dy, dx, co, ci), the entry's layout
    # torch: weight (Cin, Cout, kH, kW)
    want = F.conv_transpose2d(_t(x).permute(0, 3, 1, 2), _t(wt).permute(3, 2, 0, 1), stride=2).permute(0, 2, 3, 1).numpy()
    got = K.ref_deconv2(x, wt)
    assert got.shape == (3, 2 * h, 2 * w, co)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # the two quadrant axes are told apart: a filter that lives in (dy, dx) = (1, 0) alone lights odd rows and even columns only
    one = np.zeros_like(wt)
    one[1, 0] = wt[1, 0]
    y = K.ref_deconv2(x, one)
    assert np.abs(y[:, 1::2, 0::2]).max() > 0 and not y[:, 0::2].any() and not y[:, :, 1::2].any()


@pytest.mark.parametrize("f", K.SPLIT_FORMS + K.DECONV_FORMS + K.RES_SHIFT_FORMS[:1], ids=lambda f: f.name)
def test_column_split_and_pitches_are_plain_slicing(f):
    rng = np.random.default_rng(len(f.name))
    rows, width = (2 * f.H, 2 * f.W) if f.deconv2 else (f.OH, f.OW)
    y = rng.standard_normal((f.B, rows, width, f.Cout))
    parts = K.split_columns(f, y)
    if f.n_split:
        np.testing.assert_array_equal(np.concatenate([parts["out"], parts["out2"]], -1), y)
        assert parts["out"].shape[-1] == f.n_split
    for which, part in parts.items():
        lo = K.layout_of(f, which)
        buf, mask = K.place(part, lo)
        assert buf.shape == mask.shape == (lo["len"],) and mask.sum() == part.size
        # the same by slicing: the images, their rows, their pixels, their columns
        def carve(a):
            a = a[lo["offset"]:lo["offset"] + f.B * lo["batch_stride"]].reshape(f.B, lo["batch_stride"])
            a = a[:, :rows * lo["row_pitch"]].reshape(f.B, rows, lo["row_pitch"])
            a = a[:, :, :width * lo["pitch"]].reshape(f.B, rows, width, lo["pitch"])
            return a[..., :lo["cols"]], a[..., lo["cols"]:]
        inside, gaps = carve(buf)
        np.testing.assert_array_equal(inside, part)
        assert (gaps == K.SENTINEL).all()
        assert carve(mask)[0].all() and not carve(mask)[1].any()
        assert (buf[~mask] == K.SENTINEL).all() and (buf[:lo["offset"]] == K.SENTINEL).all()
        if lo["len"] > lo["offset"] + f.B * lo["batch_stride"]:
            assert not mask[lo["offset"] + f.B * lo["batch_stride"]:].any()
    # the layouts of the cases are what their comments say: dense pixel pitch, images further apart than a level, different fronts
    if f.n_split:
        a, b = K.layout_of(f, "out"), K.layout_of(f, "out2")
        assert a["pitch"] == f.n_split and b["pitch"] == f.Cout - f.n_split
        assert a["batch_stride"] > f.OH * f.OW * a["pitch"] and b["batch_stride"] > f.OH * f.OW * b["pitch"] and a["offset"] != b["offset"]


@pytest.mark.parametrize("f", K.SEL_FORMS, ids=lambda f: f.name)
def test_selected_class_dot_is_the_full_deconvolution_and_a_per_row_einsum(f):
    ops = K.make_operands(f)
    m = K.as_mode_sees("f32", ops)
    full = F.conv_transpose2d(_t(m["x"]).permute(0, 3, 1, 2), _t(m["w"]).permute(3, 2, 0, 1), stride=2)          # (B, C, 2H, 2W)
    full = F.relu(full * _t(m["scale"])[None, :, None, None] + _t(m["shift"])[None, :, None, None])
    cid = np.asarray(f.sel_cid)
    rows = torch.einsum("bchw,bc->bhw", full, _t(m["sel_w"])[np.maximum(cid, 0)]).reshape(f.B, -1).numpy()
    ref = K.reference(f, "f32", ops)
    assert ref["dot"].shape == (f.B, 4 * f.H * f.W)
    np.testing.assert_array_equal(ref["written"], cid >= 0)
    assert not ref["written"].all() and ref["written"].sum() >= 3
    np.testing.assert_allclose(ref["dot"][ref["written"]], rows[ref["written"]], rtol=0, atol=1e-12)
    assert (ref["abs"] >= np.abs(ref["dot"]) - 1e-12).all()
    # the bound is the one the issue derives: Cout * 2^-24 * sum |y w|, + 2^-11 * sum |y w| where y is rounded to fp16 first
    np.testing.assert_array_equal(K.selected_bound(f, "f32s", ref["abs"]), f.Cout * 2.0 ** -24 * ref["abs"])
    np.testing.assert_array_equal(K.selected_bound(f, "f16", ref["abs"]), (f.Cout * 2.0 ** -24 + 2.0 ** -11) * ref["abs"])


def test_whole_layer_against_torch_on_every_plain_case():
    """ref_layer (conv or scatter, scale / shift, shifted residual, activation) against the same chain of torch operations."""
    for f in K.RES_SHIFT_FORMS + K.STRIDED_FORMS + K.DECONV_FORMS[:2]:
        ops = K.make_operands(f)
        m = K.as_mode_sees("f32s", ops)
        if f.deconv2:
            y = F.conv_transpose2d(_t(m["x"]).permute(0, 3, 1, 2), _t(m["w"]).permute(3, 2, 0, 1), stride=2)
        else:
            y = F.conv2d(_t(m["x"][:, ::f.in_step, ::f.in_step]).permute(0, 3, 1, 2), _t(m["w"]).permute(0, 3, 1, 2), stride=f.stride, padding=f.k // 2)
        y = y * _t(m["scale"])[None, :, None, None] + _t(m["shift"])[None, :, None, None]
        if f.res_shift >= 0:
            up = _t(m["res"]).permute(0, 3, 1, 2)
            if f.res_shift:
                up = up.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)[:, :, :f.OH, :f.OW]
            y = y + up
        if f.act == 1:
            y = F.relu(y)
        np.testing.assert_allclose(K.ref_layer(f, m), y.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-11, err_msg=f.name)


def test_operand_rounding_follows_the_modes():
    f = K.RES_SHIFT_FORMS[3]
    ops = K.make_operands(f)
    h = lambda a: a.astype(np.float16).astype(np.float64)
    for mode in K.MODES:
        m = K.as_mode_sees(mode, ops)
        np.testing.assert_array_equal(m["x"], h(ops["x"]) if mode == "f16" else ops["x"].astype(np.float64))
        np.testing.assert_array_equal(m["res"], h(ops["res"]) if mode == "f16" else ops["res"].astype(np.float64))
        np.testing.assert_array_equal(m["w"], ops["w"].astype(np.float64) if mode == "f32" else h(ops["w"]))
        np.testing.assert_array_equal(m["scale"], ops["scale"].astype(np.float64))


def test_single_image_forms_are_the_batch_forms_image():
    f = K.SEL_FORMS[0]
    g = f.image(2)
    assert g.B == 1 and g.sel_cid == (f.sel_cid[2],) and g.H == f.H
    ops = K.make_operands(f)
    one = K.image_operands(ops, 2)
    np.testing.assert_array_equal(one["x"][0], ops["x"][2])
    assert one["w"] is ops["w"]
