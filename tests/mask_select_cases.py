"""Cases of the mask head's row selection (csrc/kernels_elementwise.hip: k_mask_row_flags, k_mask_row_compact and the three tails) and THE
definition they are held to: a plain numpy restatement of the rule, written here from the rule.

The rule (TimeDistributedMaskLayer.swift:58-89 behind MultiArrayBatchProvider(removeZeros: true)):
  * a pooled row is kept iff every element is != 0 (a NaN is != 0: kept; -0.0 is not: dropped);
  * the kept rows are compacted, mapping[i] = the row compact index i came from, nk = their number;
  * compact index i is written to output row mapping[i] with the class of DETECTION ROW i — int(det[i, 4]) truncated toward zero, clamped
    to [0, nc - 1] — not the class of row mapping[i];
  * rows from nk onward are then zeroed over their whole stride, so a write to a row mapping[i] >= nk is lost;
  * a row below nk that nothing maps to is never written.

No GPU, no HIP library and no oracle library here.  tests/test_mask_select_cases_host.py proves from the definition alone that every case
is what its comment claims (and pins the definition against the oracle's orc_mask_layer_write); tests/test_gpu_mask_select.py sends the same
arrays through mrcnn_test_mask_select_batch.  Everything is seeded: the two files see the same arrays.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

F = np.float32
NC = 5
D = 9
SENTINEL = F(-777.0)           # no sigmoid and no plane value of the cases comes near it
U24 = 2.0 ** -24

# one batch of six images; kept = 9, 0, 4, 3, 8, 1
PATTERNS = np.array([
    [1, 1, 1, 1, 1, 1, 1, 1, 1],     # 0: identity mapping
    [0, 0, 0, 0, 0, 0, 0, 0, 0],     # 1: kept = 0, every row zeroed, sel_cid all -1
    [1, 0, 1, 1, 0, 1, 0, 0, 0],     # 2: nk = 4, mapping 0,2,3,5: rows 2 / 3 carry the classes of detections 1 / 2, the write to row 5 is lost,
                                     #    row 1 (below nk, nothing maps to it) is never written, row 4 is zeroed
    [0, 0, 0, 1, 1, 1, 0, 0, 0],     # 3: every mapping[i] >= nk = 3: nothing written, rows 0-2 untouched, rows 3-8 zero
    [1, 1, 1, 1, 1, 1, 1, 1, 0],     # 4: a kept prefix under the class values of CLAMP_CLASSES
    [0, 0, 0, 0, 0, 0, 0, 0, 1],     # 5: only the last row kept: mapping[0] = 8 >= nk = 1, nothing written, row 0 untouched
], np.int32)
B = PATTERNS.shape[0]
# the same kept counts as prefixes: what a predict on random weights produces (valid rows first, padding behind)
PREFIX_PATTERNS = (np.arange(D)[None, :] < PATTERNS.sum(1)[:, None]).astype(np.int32)
# image 4, detection rows 0..7 (row 8 is dropped).  No NaN: the float -> int conversion of a NaN is not defined in C++.
CLAMP_CLASSES = (-3.0, -0.5, 2.9, NC - 1, NC, NC + 1000, 1e9, -1e9)
IMAGE2_CLASSES = (1, 3, 0, 2, 4, 1, 3, 0, 2)        # detections 0..4 all different


# ------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------
def keep_flags(rows):
    """removeZeros: rows (..., row_len) as the kernel reads them (already rounded to its element type) -> 1 where every element is != 0."""
    return (np.asarray(rows) != 0).all(-1).astype(np.int32)


def class_of(v, nc):
    """int(v) truncated toward zero, clamped to [0, nc - 1]; v is the fp32 the detection row holds."""
    return min(max(int(np.trunc(float(F(v)))), 0), nc - 1)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


@dataclass
class Expect:
    mapping: np.ndarray       # (nk,) int: the defined entries of the mapping row
    kept: int
    sel_cid: np.ndarray       # (R,) int: the class whose value stands in the row, -1 where the rule leaves or zeroes it
    written: np.ndarray       # (R, out_stride) bool: the elements the rule writes
    values: np.ndarray        # (R, out_stride) float64: what it writes there (NaN where it writes nothing)


def define_image(flags, det, z, out_stride=None, det_rows=None, activate=True, class_from="compact", zero="from_nk"):
    """One image.  flags (D,), det (R, >= 6) with R >= D, z (D, nc, HW) float64 = per row and per class the pre-activation (activate) or the
    plane value (activate = False).  The loops are the rule's, in its order: the writes, then the zero padding over them.
    class_from / zero select a deliberately WRONG reading (tests/test_mask_select_cases_host.py):
      class_from "actual"   the class of det[mapping[i]] instead of det[i];
      zero "dropped"        the D - nk rows whose flag is 0 are zeroed instead of the rows from nk onward;
      zero "from_D_minus_nk" the rows from D - nk onward are zeroed."""
    flags, det, z = np.asarray(flags), np.asarray(det), np.asarray(z, np.float64)
    d, nc, hw = z.shape
    rows = det.shape[0] if det_rows is None else det_rows
    stride = hw if out_stride is None else out_stride
    assert flags.shape == (d,) and rows >= d and stride >= hw and det.shape[0] >= rows
    mapping = [r for r in range(d) if flags[r]]
    nk = len(mapping)
    written = np.zeros((rows, stride), bool)
    values = np.full((rows, stride), np.nan)
    sel = np.full(rows, -1, np.int64)
    for i, actual in enumerate(mapping):
        cid = class_of(det[actual if class_from == "actual" else i, 4], nc)
        values[actual, :hw] = sigmoid(z[actual, cid]) if activate else z[actual, cid]
        written[actual, :hw] = True
        sel[actual] = cid
    if zero == "from_nk":
        zeroed = np.arange(rows) >= nk
    elif zero == "dropped":
        zeroed = np.concatenate([flags == 0, np.ones(rows - d, bool)])
    else:
        zeroed = np.arange(rows) >= d - nk
    values[zeroed] = 0.0
    written[zeroed] = True
    sel[zeroed] = -1
    return Expect(np.asarray(mapping, np.int64), nk, sel, written, values)


def define_batch(flags, det, z, **kw):
    return [define_image(flags[b], det[b], z[b], **kw) for b in range(len(flags))]


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """What one call of mrcnn_test_mask_select_batch takes (float32 / int32, C order) and the shapes that go with it."""
    name: str
    form: int
    flags: np.ndarray                 # (B, D) int32
    det: np.ndarray                   # (B, R, det_stride)
    hw: int
    nc: int = NC
    dtype: str = "f32"
    out_stride: int = 0
    ops: dict = field(default_factory=dict)       # form 0: feat (B,D,HW,C), w (nc,C), bias; form 1: per_class (B,D,nc,HW,parts), bias; form 2: masks (B,D,nc,HW)

    @property
    def batch(self):
        return self.flags.shape[0]

    @property
    def d(self):
        return self.flags.shape[1]

    @property
    def det_rows(self):
        return self.det.shape[1]

    def image(self, b):
        """The same call on image b alone."""
        ops = {k: (v if k in ("w", "bias") else v[b:b + 1]) for k, v in self.ops.items()}
        return Case(f"{self.name}[{b}]", self.form, self.flags[b:b + 1], self.det[b:b + 1], self.hw, self.nc, self.dtype, self.out_stride, ops)


def as_dtype_sees(a, dtype):
    """float64 copy of a float32 operand as the kernel reads it: rounded to fp16 on the host in the fp16 mode."""
    a = np.asarray(a, F)
    return (a.astype(np.float16) if dtype == "f16" else a).astype(np.float64)


def make_det(flags, det_rows, det_stride, seed, image2_like=(2,), clamp_image=4):
    """(B, det_rows, det_stride): boxes in [0, 1), the class in column 4, score 0.9, and — det_stride 7 — a column 6 holding another class + 0.5,
    so that a row read at the wrong stride or the wrong column takes a wrong class.  Neighbouring rows never share a class."""
    rng = np.random.default_rng(seed)
    nb = flags.shape[0]
    det = np.zeros((nb, det_rows, det_stride), F)
    det[..., :4] = rng.random((nb, det_rows, 4))
    r = np.arange(det_rows)
    for b in range(nb):
        det[b, :, 4] = (3 * r + 1 + b) % NC
        if b in image2_like:
            det[b, :len(IMAGE2_CLASSES), 4] = IMAGE2_CLASSES[:det_rows]
        if b == clamp_image:
            det[b, :len(CLAMP_CLASSES), 4] = CLAMP_CLASSES
    det[..., 5] = 0.9
    if det_stride > 6:
        det[..., 6:] = ((np.clip(det[..., 4:5], 0, NC - 1).astype(np.int64) + 2) % NC + 0.5).astype(F)
    return det


def preact(case):
    """Per row and per class what the definition selects from, in float64, as the kernels of the case's form see their operands:
      form 0: z = sum_c x_c w_c + bias in float64 over the dtype-rounded feat, and mag = sum_c |x_c w_c| for the error bound;
      form 1: z = the float32 sequential sum h = 0 .. parts-1 of the partial dots, then + bias — adds only, so numpy reproduces the kernel's bits;
      form 2: the planes themselves.
    -> (z (B, D, nc, HW), mag or None)"""
    o = case.ops
    if case.form == 0:
        x, w = as_dtype_sees(o["feat"], case.dtype), o["w"].astype(np.float64)
        z = np.einsum("bdpc,nc->bdnp", x, w) + o["bias"].astype(np.float64)[None, None, :, None]
        return z, np.einsum("bdpc,nc->bdnp", np.abs(x), np.abs(w))
    if case.form == 1:
        p = o["per_class"]
        s = p[..., 0].copy()
        for h in range(1, p.shape[-1]):
            s = (s + p[..., h]).astype(F)
        return (s + o["bias"][None, None, :, None]).astype(F).astype(np.float64), None
    return o["masks"].astype(np.float64), None


def expect(case, **wrong):
    """The definition over the batch of a case -> ([Expect per image], z, mag)."""
    z, mag = preact(case)
    return define_batch(case.flags, case.det, z, out_stride=case.out_stride or case.hw, activate=case.form != 2, **wrong), z, mag


def partial_for(case, sel_cid):
    """Form 1: what the deconvolution's selected-class epilogue leaves given the class table sel_cid (B, >= D): the partial dots of the row's class;
    NaN in the rows of class -1, which the tail must not read."""
    p = case.ops["per_class"]
    nb, d = p.shape[:2]
    out = np.full((nb, d) + p.shape[3:], np.nan, F)
    for b in range(nb):
        for r in range(d):
            if sel_cid[b][r] >= 0:
                out[b, r] = p[b, r, sel_cid[b][r]]
    return out


def _class_row_offsets(nb, d, nc):
    """O(1) steps between classes and between rows: a wrong class or a wrong row moves a sigmoid by far more than any rounding bound."""
    cls = 1.0 * (np.arange(nc) - (nc - 1) / 2)
    row = 0.5 * ((3 * np.arange(d)[None, :] + np.arange(nb)[:, None]) % 5 - 2)
    return cls[None, None, :] + row[:, :, None]                                   # (nb, d, nc)


def make_case(form, hw, *, c=0, parts=0, dtype="f32", flags=PATTERNS, out_extra=0, det_stride=6, det_extra=0, seed=0, name=None, **det_kw):
    """One call on `flags` (default: the batch of six).  form 0: feat ~ N(0, 1), w ~ N(0, 1 / C), bias = the class step; forms 1 and 2: per row,
    class and pixel the class / row steps plus noise (form 1: spread over `parts` partial dots of different size)."""
    flags = np.ascontiguousarray(flags, np.int32)
    nb, d = flags.shape
    rng = np.random.default_rng(1000 * form + 7 * hw + 13 * c + parts + seed)
    det = make_det(flags, d + det_extra, det_stride, seed + 1, **det_kw)
    step = _class_row_offsets(nb, d, NC)
    if form == 0:
        ops = {"feat": rng.standard_normal((nb, d, hw, c)).astype(F), "w": (rng.standard_normal((NC, c)) / np.sqrt(c)).astype(F),
               "bias": (1.0 * (np.arange(NC) - 2)).astype(F)}
    elif form == 1:
        z = step[..., None] + 0.25 * rng.standard_normal((nb, d, NC, hw))
        share = rng.dirichlet(np.ones(parts), (nb, d, NC, hw)) if parts > 1 else np.ones((nb, d, NC, hw, 1))
        ops = {"per_class": (z[..., None] * share + (rng.standard_normal(share.shape) if parts > 1 else 0.0)).astype(F),
               "bias": (0.125 * np.arange(NC) - 0.3).astype(F)}
    else:
        ops = {"masks": (step[..., None] + 0.25 * rng.standard_normal((nb, d, NC, hw))).astype(F)}
    return Case(name or f"form{form}-hw{hw}-c{c}-parts{parts}-{dtype}-det{det_stride}+{det_extra}rows-out+{out_extra}", form, flags, det, hw, NC, dtype, hw + out_extra if out_extra else 0, ops)


# the calls of tests/test_gpu_mask_select.py: the smallest shapes at which each kernel's loops take every branch
#   form 0: 49 x 4 waves cover 196 pixels a step: HW 1 (below), 197 (one past), 785 (several steps); C 4: one lane active, 260: lane 0 takes a second
#           trip of the c += 256 loop
_LAYOUTS = (dict(), dict(out_extra=3, det_stride=7))         # dense as the engine binds it | out_stride = HW + 3 and det_stride = 7
FORM0 = [dict(hw=hw, c=c, **_LAYOUTS[(i + j) % 2]) for i, hw in enumerate((1, 197, 785)) for j, c in enumerate((4, 260))]
#   form 1: 256 pixels per block: HW 1 and 257 (a second block with one pixel)
FORM1 = [dict(hw=hw, parts=parts, **_LAYOUTS[(i + j) % 2]) for i, hw in enumerate((1, 257)) for j, parts in enumerate((1, 2, 4))]
#   form 2: 256 threads stride a row: HW 1 and 257; det_rows = D + 2: the padding runs on to the detection count
FORM2 = [dict(hw=hw, det_extra=extra, **_LAYOUTS[(i + j) % 2]) for i, hw in enumerate((1, 257)) for j, extra in enumerate((0, 2))]


def form0_cases():
    return [make_case(0, dtype=dt, **kw) for kw in FORM0 for dt in ("f32", "f16")]


def form1_cases():
    return [make_case(1, **kw) for kw in FORM1]


def form2_cases():
    return [make_case(2, **kw) for kw in FORM2]


def wide_flags():
    """(2, 130): image 0 drops row 64 alone — kept = 129, mapping[i] = i + 1 from i = 64 on, compact indices 128 (a second trip of
    k_mask_select_classes' 128-thread loop) maps to row 129 >= nk: lost; row 64 is never written, row 129 zeroed.  Image 1 drops every third row."""
    f = np.ones((2, 130), np.int32)
    f[0, 64] = 0
    f[1, ::3] = 0
    return f


def wide_case():
    return make_case(1, 5, parts=2, flags=wide_flags(), name="form1-D130", image2_like=(), clamp_image=-1)


# ------------------------------------------------------------------------------------------------
# the predicate on pooled rows
# ------------------------------------------------------------------------------------------------
ROW_LENS = (1, 255, 256, 257, 700)
ROW_KINDS = ("zero_first", "zero_last", "zero_at_256", "minus_zero", "nan", "no_zero", "subnormal_f16", "tiny")
PRED_BATCH = 3


@functools.lru_cache(maxsize=None)
def pooled_rows(row_len):
    """(3, 8, row_len + 5) float32: elements of magnitude in [0.5, 2) (fp16 holds them), the 5 elements behind a row ZERO (they must not be read),
    and per image the eight ROW_KINDS in an order of its own:
      zero_first / zero_last / zero_at_256   a single 0 at index 0 / row_len - 1 / 256 (a row that does not reach 256 has no zero: kept)
      minus_zero      a single -0.0: dropped          nan      a single NaN: kept          no_zero   kept
      subnormal_f16   a single 2^-24, the smallest fp16 subnormal: kept in both types
      tiny            a single 1e-8: kept in fp32, dropped in fp16, where the host rounding makes it zero.
    -> (rows, kinds (3, 8) of names)"""
    rng = np.random.default_rng(500 + row_len)
    n = len(ROW_KINDS)
    rows = np.zeros((PRED_BATCH, n, row_len + 5), F)
    rows[..., :row_len] = (0.5 + 1.5 * rng.random((PRED_BATCH, n, row_len))) * rng.choice([-1.0, 1.0], (PRED_BATCH, n, row_len))
    kinds = np.empty((PRED_BATCH, n), object)
    for b in range(PRED_BATCH):
        for r in range(n):
            kind = ROW_KINDS[(r * 3 + b * 5 + 1) % n]          # 3 and 8 are coprime: every kind once per image, at another row in each
            kinds[b, r] = kind
            at = int(rng.integers(row_len))
            if kind == "zero_first":
                rows[b, r, 0] = 0.0
            elif kind == "zero_last":
                rows[b, r, row_len - 1] = 0.0
            elif kind == "zero_at_256" and row_len > 256:
                rows[b, r, 256] = 0.0
            elif kind == "minus_zero":
                rows[b, r, at] = -0.0
            elif kind == "nan":
                rows[b, r, at] = np.nan
            elif kind == "subnormal_f16":
                rows[b, r, at] = 2.0 ** -24
            elif kind == "tiny":
                rows[b, r, at] = 1e-8
    rows.setflags(write=False)
    return rows, kinds


def predicate_expect(row_len, dtype):
    """The flags the predicate must give, from the definition on the dtype-rounded rows (the gap excluded)."""
    rows, _ = pooled_rows(row_len)
    return keep_flags(as_dtype_sees(rows[..., :row_len], dtype))


def predicate_case(row_len):
    """A form-2 call (HW = 1) whose flags come from the pooled rows; case.flags is left for the test to fill from predicate_expect."""
    rows, _ = pooled_rows(row_len)
    return make_case(2, 1, flags=np.zeros(rows.shape[:2], np.int32), seed=row_len, name=f"pooled-{row_len}", image2_like=(), clamp_image=-1)
