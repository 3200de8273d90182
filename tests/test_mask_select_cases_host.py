"""The cases of tests/mask_select_cases.py are what their comments claim — proved from the definition alone, on the CPU — and the definition
is the rule: it agrees with the oracle's orc_mask_valid_rows / orc_mask_layer_write (the only check here that needs the oracle library;
tests/test_gpu_mask_select.py needs none).

The two readings a kernel could take without the earlier suite noticing — the class of det[mapping[i]] instead of det[i], and zeroing the
D - nk dropped rows instead of the rows from nk onward — give another write set or values more than 0.1 away on the new batch, and EXACTLY the
right result on prefix patterns (valid rows first, padding behind: what a predict on random weights produces but for a stray dropped
row).  A third reading, zeroing the rows from D - nk onward, is caught by the new batch as well; it differs on prefixes too, so the earlier
suite was not blind to it."""
import numpy as np
import pytest

import mask_select_cases as K

WRONG = [dict(class_from="actual"), dict(zero="dropped")]


def small(form=2, hw=3, **kw):
    return K.make_case(form, hw, **({"parts": 2} if form == 1 else {"c": 8} if form == 0 else {}), **kw)


def differs(a, b):
    """Two expectations of one image disagree: another write set, or some value more than 0.1 away."""
    if not np.array_equal(a.written, b.written):
        return True
    return bool((np.abs(a.values - b.values)[a.written] > 0.1).any())


def test_image_2_crosses_class_and_row_loses_a_write_and_leaves_a_row():
    case = small()
    e = K.expect(case)[0][2]
    det_cls = [K.class_of(v, K.NC) for v in case.det[2, :, 4]]
    assert e.kept == 4 and list(e.mapping) == [0, 2, 3, 5]
    crossed = [(i, r) for i, r in enumerate(e.mapping) if r < e.kept and i != r and det_cls[i] != det_cls[r]]
    assert (1, 2) in crossed and (2, 3) in crossed                       # row 2 carries detection 1's class, row 3 detection 2's
    assert list(e.sel_cid) == [det_cls[0], -1, det_cls[1], det_cls[2], -1, -1, -1, -1, -1]
    assert len(set(det_cls[:5])) == 5
    assert not e.written[1].any()                                        # below nk, nothing maps to it
    assert e.written[4:].all() and (e.values[4:] == 0).all()             # 4 is invalid and at nk; 5 was written and zeroed over
    z = K.preact(case)[0][2]
    np.testing.assert_array_equal(e.values[2], z[2, det_cls[1]])
    assert np.abs(z[2, det_cls[1]] - z[2, det_cls[2]]).min() > 0.1         # the two classes' planes are far apart


def test_images_3_and_5_write_nothing_and_image_1_zeroes_everything():
    e = K.expect(small())[0]
    for b, nk in ((3, 3), (5, 1)):
        assert e[b].kept == nk and (e[b].mapping >= nk).all()
        assert not e[b].written[:nk].any() and e[b].written[nk:].all() and (e[b].values[nk:] == 0).all()
        assert (e[b].sel_cid == -1).all()
    assert e[1].kept == 0 and e[1].written.all() and (e[1].values == 0).all() and (e[1].sel_cid == -1).all()
    assert e[0].kept == K.D and list(e[0].mapping) == list(range(K.D)) and (e[0].sel_cid >= 0).all()
    assert all(a != b for a, b in zip(e[0].sel_cid[:-1], e[0].sel_cid[1:]))


def test_image_4_hits_both_sides_of_the_clamp():
    case = small()
    raw = [int(np.trunc(float(v))) for v in case.det[4, :8, 4]]
    assert min(raw) < 0 and max(raw) >= K.NC and raw[1] == 0 and raw[2] == 2                   # -0.5 -> 0 and 2.9 -> 2: truncation, not rounding
    assert np.isfinite(case.det[..., 4]).all()
    assert list(K.expect(case)[0][4].sel_cid) == [0, 0, 2, K.NC - 1, K.NC - 1, K.NC - 1, K.NC - 1, 0, -1]
    assert all(abs(v) < 2 ** 31 for v in raw)                           # the conversion to int is defined for every value


def test_kept_takes_0_and_D_and_four_other_values():
    kept = [x.kept for x in K.expect(small())[0]]
    assert 0 in kept and K.D in kept and len(set(kept) - {0, K.D}) >= 3 and len(set(kept)) == K.B


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("wrong", WRONG + [dict(zero="from_D_minus_nk")], ids=lambda w: "-".join(w.values()))
def test_a_wrong_definition_is_caught_by_the_new_batch(form, wrong):
    case = small(form, out_extra=3, det_stride=7)
    right, bad = K.expect(case)[0], K.expect(case, **wrong)[0]
    caught = [b for b in range(K.B) if differs(right[b], bad[b])]
    assert 2 in caught, (wrong, caught)


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("wrong", WRONG, ids=lambda w: "-".join(w.values()))
def test_prefix_patterns_alone_cannot_tell_the_wrong_definitions_from_the_right_one(form, wrong):
    """Why the whole-model predicts could not see the difference: with the valid rows in front, mapping is the identity."""
    case = small(form, flags=K.PREFIX_PATTERNS)
    right, bad = K.expect(case)[0], K.expect(case, **wrong)[0]
    for b in range(K.B):
        np.testing.assert_array_equal(right[b].written, bad[b].written)
        np.testing.assert_array_equal(right[b].values, bad[b].values)
        np.testing.assert_array_equal(right[b].sel_cid, bad[b].sel_cid)


def test_layouts_strides_and_the_wide_case():
    for cases in (K.form0_cases(), K.form1_cases(), K.form2_cases()):
        assert any(c.out_stride == c.hw + 3 and c.det.shape[2] == 7 for c in cases)
        assert len({c.name for c in cases}) == len(cases)
    assert any(c.det_rows == K.D + 2 for c in K.form2_cases())
    assert {(c.hw, c.ops["feat"].shape[-1], c.dtype) for c in K.form0_cases()} == {(h, c, t) for h in (1, 197, 785) for c in (4, 260) for t in ("f32", "f16")}
    assert {(c.hw, c.ops["per_class"].shape[-1]) for c in K.form1_cases()} == {(h, p) for h in (1, 257) for p in (1, 2, 4)}
    # detection column 6 would give another class than column 4 in every row
    c = K.form2_cases()[1]
    assert c.det.shape[2] == 7
    assert all(K.class_of(a, K.NC) != K.class_of(b, K.NC) for a, b in zip(c.det[..., 4].ravel(), c.det[..., 6].ravel()))
    # D = 130: one hole, kept = 129; compact index 128 is lost, row 64 never written, the classes of neighbours differ
    w = K.wide_case()
    e = K.expect(w)[0]
    assert w.d == 130 and e[0].kept == 129 and e[0].mapping[128] == 129 and not e[0].written[64].any() and e[0].written[129].all()
    assert e[0].sel_cid[64] == -1 and e[0].sel_cid[128] == K.class_of(w.det[0, 127, 4], K.NC) != K.class_of(w.det[0, 128, 4], K.NC)
    assert e[1].kept not in (0, 129, 130) and differs(e[0], K.expect(w, class_from="actual")[0][0])


@pytest.mark.parametrize("row_len", K.ROW_LENS)
def test_predicate_rows_are_what_their_names_say(row_len):
    rows, kinds = K.pooled_rows(row_len)
    assert rows.shape == (K.PRED_BATCH, len(K.ROW_KINDS), row_len + 5) and (rows[..., row_len:] == 0).all()
    f32, f16 = K.predicate_expect(row_len, "f32"), K.predicate_expect(row_len, "f16")
    want32 = {"zero_first": 0, "zero_last": 0, "zero_at_256": int(row_len <= 256), "minus_zero": 0, "nan": 1, "no_zero": 1, "subnormal_f16": 1, "tiny": 1}
    for b in range(K.PRED_BATCH):
        assert sorted(kinds[b]) == sorted(K.ROW_KINDS)
        for r, kind in enumerate(kinds[b]):
            assert f32[b, r] == want32[kind], (b, r, kind)
            assert f16[b, r] == (0 if kind == "tiny" else want32[kind]), (b, r, kind)
            body = rows[b, r, :row_len]
            assert (body == 0).sum() == (0 if want32[kind] else 1)            # one zero at the most: the row hangs on that element alone
            if kind == "zero_at_256" and row_len > 256:
                assert body[256] == 0
            if kind == "minus_zero":
                assert np.signbit(body[body == 0]).all()
    assert len({tuple(k) for k in kinds}) == K.PRED_BATCH and len({tuple(f) for f in f32}) == K.PRED_BATCH


def test_the_definition_agrees_with_the_oracle_on_image_2(orc):
    """orc_mask_valid_rows on rows that are zero where the flag is, orc_mask_layer_write on the kept rows' planes."""
    case = small(2, hw=6)
    b = 2
    z = K.preact(case)[0][b]
    pooled = np.where(case.flags[b][:, None] != 0, np.float32(1.5), np.float32(0.0)) * np.ones((1, 4), np.float32)
    mapping = orc.mask_valid_rows(pooled)
    e = K.define_image(case.flags[b], case.det[b], z, activate=False)
    np.testing.assert_array_equal(mapping, e.mapping)
    np.testing.assert_array_equal(K.keep_flags(pooled), case.flags[b])
    out = np.full((case.det_rows, case.hw), K.SENTINEL, np.float32)
    orc.mask_layer_write(z[mapping], mapping, np.ascontiguousarray(case.det[b]), out)
    np.testing.assert_array_equal(out != K.SENTINEL, e.written)
    np.testing.assert_array_equal(out[e.written], e.values[e.written].astype(np.float32))
    for wrong in WRONG:                                                   # and the oracle sides with the right reading
        assert differs(e, K.define_image(case.flags[b], case.det[b], z, activate=False, **wrong))
