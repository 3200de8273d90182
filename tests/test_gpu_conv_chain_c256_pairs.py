"""The ring form of the chained pair at C = 256 (kernels_conv_chain.hip) where its wave pairs and their hand-over can go wrong.

A block of the ring form owns 128 rows and has eight waves: the two waves of a SIMD share 32 rows, one multiplying P's sums and issuing the
block's DMAs, the other running P's epilogue and Q, with one block barrier per 32-column piece between them.  A pair whose rows lie beyond M
keeps the barriers and the DMAs going and does nothing else; a pair with fewer than 32 rows takes the path with row tests.  The launch is a
policy, so every case must agree with conv_forward x 2 BIT FOR BIT (tests/test_gpu_conv_chain.py's case maker and comparison, as
tests/test_gpu_conv_chain_c256.py uses them; the two launches themselves are held against float64 there).
"""
import functools

import numpy as np
import pytest

import test_gpu_conv_chain as base

pytestmark = pytest.mark.gpu

C = 256
FP16_LIMIT = base.FP16_LIMIT
# B, H, W with B * H * W = M —
#   128: one exactly full block;  129: a second block with one row, and three pairs that only keep the ring going;
#   33: one full pair and a one-row pair;  97: three full pairs and a one-row pair;  255: the last pair is one row short
CASES = [(2, 8, 8), (1, 3, 43), (1, 3, 11), (1, 1, 97), (1, 15, 17)]
RACE = (2, 12, 12)          # M = 288: two full blocks and a ragged one


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    return base.make(C, B, H, W, False, seed=C + 11 * B + H + 3 * W)


@functools.lru_cache(maxsize=None)
def _two_launches(B, H, W, dtype, in_place):
    y, t1, flag = base.chain(_case(B, H, W), dtype, False, in_place)
    y.setflags(write=False); t1.setflags(write=False)
    return y, t1, flag


def test_the_shapes_are_the_row_counts_they_claim():
    assert [b * h * w for b, h, w in CASES] == [128, 129, 33, 97, 255] and RACE[0] * RACE[1] * RACE[2] == 288


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("B,H,W", CASES)
def test_chained_equals_the_two_launches_bitwise(B, H, W, dtype, in_place):
    y0, t0, f0 = _two_launches(B, H, W, dtype, in_place)
    y1, t1, f1 = base.chain(_case(B, H, W), dtype, True, in_place)
    assert np.isfinite(y1).all() and np.isfinite(t1).all()
    assert (y0 == 0).mean() > 0.1 and (t0 == 0).mean() > 0.1 and (y0 > 0).mean() > 0.1 and (t0 > 0).mean() > 0.1      # ReLU cuts a good share of both
    base._same_bits(y1, y0, "y")
    base._same_bits(t1, t0, "t1")
    assert f1 == f0 == 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
@pytest.mark.parametrize("where", ["y", "t1"])
def test_a_watchdog_plant_in_the_last_piece_of_the_last_live_pair(where, dtype):
    """M = 97: the block's last live pair owns row 96 alone.  The plant sits in the last chunk's second piece (columns 992 .. 1023 of y): for y a
    residual element past the fp16 range; for t1 a y element just inside the range that one of Q's filter elements carries past it."""
    b = _case(1, 1, 97)
    row, col, ch = 96, 4 * C - 24, C - 5
    hot = dict(b)
    hot["x"] = b["x"].copy()
    hot["s3"] = np.abs(b["s3"])
    if where == "y":
        hot["x"][0, 0, row, col] = 70000.0
    else:
        hot["x"][0, 0, row, col] = 60000.0
        hot["w1"] = b["w1"].copy()
        hot["w1"][ch, col] = 4.0
        hot["s1"] = b["s1"].copy()
        hot["s1"][ch] = 1.0
    y0, t0, f0 = base.chain(hot, dtype, False, 1)
    y1, t1, f1 = base.chain(hot, dtype, True, 1)
    if where == "y":
        assert (np.abs(y0) >= FP16_LIMIT).sum() == 1 and abs(y0[0, 0, row, col]) >= FP16_LIMIT
    else:
        assert np.abs(y0).max() < FP16_LIMIT and (np.abs(t0) >= FP16_LIMIT).sum() == 1 and abs(t0[0, 0, row, ch]) >= FP16_LIMIT
    base._same_bits(y1, y0, where + ": y")
    base._same_bits(t1, t0, where + ": t1")
    assert f0 == 1 and f1 == 1, (where, f0, f1)
    # and without the plant the same rows raise nothing
    assert _two_launches(1, 1, 97, dtype, 1)[2] == 0


@pytest.mark.parametrize("dtype", ["f32x3", "f32s"])
def test_twenty_chained_launches_give_the_same_bits(dtype):
    """hand-over races: a piece read before its barrier, or a stage overwritten while it is read, would change bits from run to run"""
    y0, t0, f0 = _two_launches(*RACE, dtype, 0)
    for i in range(20):
        y1, t1, f1 = base.chain(_case(*RACE), dtype, True, 0)
        base._same_bits(y1, y0, f"run {i}: y")
        base._same_bits(t1, t0, f"run {i}: t1")
        assert f1 == f0 == 0
