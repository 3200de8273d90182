"""The engine-only forms of the convolution family (ConvDesc, csrc/kernels.h): their cases and ONE float64 definition per form.

Shared by tests/test_conv_forms_host.py, which pins each definition here against an independent statement on the CPU, and
tests/test_gpu_conv_forms.py, which holds the kernels to them through mrcnn_test_conv_form_nhwc.  Everything is plain numpy on
float64; the definitions are written as index arithmetic (the way the epilogues address memory), the host test restates them
with library operations (conv2d, conv_transpose2d, repeat_interleave, slicing, einsum).
"""
from dataclasses import dataclass, replace

import numpy as np

MODES = ("f16", "f32", "f32s", "f32x3")
# |got - ref|.max() <= TOL * max(1, |ref|.max()): the figures of tests/test_gpu_conv_kernels.py
TOL = {"f16": 2e-3, "f32": 2e-5, "f32s": 2e-5, "f32x3": 1e-5}
SENTINEL = -777.0            # fp16 holds it; no activated output of the cases' data comes near it


@dataclass(frozen=True)
class Layout:
    """Where an output's images sit in its buffer, as distances ON TOP of the dense ones."""
    offset: int = 0          # elements in front of image 0
    gap: int = 0             # elements between two images
    pitch_extra: int = 0     # unused elements behind a pixel's columns
    row_extra: int = 0       # deconv2 only: unused elements behind an output row
    tail: int = 0            # elements behind the last image


@dataclass(frozen=True)
class Form:
    name: str
    B: int
    H: int                   # the level the layer READS (the caller's tensor is H * in_step x W * in_step)
    W: int
    Cin: int
    Cout: int
    k: int = 1
    stride: int = 1
    act: int = 0
    in_step: int = 1
    res_shift: int = -1      # -1: no residual; 0: dense; 1: read at (oh >> 1, ow >> 1)
    n_split: int = 0
    deconv2: bool = False
    out_f32: bool = False    # applies in f16 (the other modes store fp32 anyway)
    nc: int = 0              # > 0: selected-class mode
    sel_cid: tuple = ()
    out: Layout = Layout()
    out2: Layout = Layout()

    @property
    def OH(self):
        return (self.H + 2 * (self.k // 2) - self.k) // self.stride + 1

    @property
    def OW(self):
        return (self.W + 2 * (self.k // 2) - self.k) // self.stride + 1

    def image(self, b):
        """The same layer over image (ROI row) b alone."""
        return replace(self, B=1, sel_cid=self.sel_cid[b:b + 1])


RES_SHIFT_FORMS = [
    Form("lateral_odd_level", 3, 13, 10, 64, 256, res_shift=1),          # M = 390 = 3.05 tiles; image boundaries inside tiles; two N tiles
    Form("lateral_24x24", 2, 24, 24, 128, 256, res_shift=1),             # not a power of two: tiles start mid-row; K long enough for the ping-pong kernel
    Form("lateral_36_columns", 5, 6, 6, 64, 36, res_shift=1),            # vector epilogue on fp32 tensors, scalar on fp16
    Form("lateral_30_columns", 2, 9, 7, 64, 30, res_shift=1),            # scalar everywhere; odd level
    Form("lateral_3x3", 2, 12, 10, 64, 128, k=3, res_shift=1),
    Form("lateral_relu", 3, 13, 10, 64, 256, act=1, res_shift=1),
]
# na = 3: 6 logits + 12 deltas per pixel, dense pixel pitches, batch strides of a concatenated buffer with other levels in front
SPLIT_FORMS = [
    Form("rpn_heads_cin64", 3, 5, 7, 64, 18, n_split=6, out_f32=True, out=Layout(offset=10, gap=24, tail=5), out2=Layout(offset=7, gap=36, tail=3)),
    Form("rpn_heads_cin512", 3, 5, 7, 512, 18, n_split=6, out_f32=True, out=Layout(offset=10, gap=24, tail=5), out2=Layout(offset=7, gap=36, tail=3)),
]
STRIDED_FORMS = [
    Form("p6_view_3x3", 2, 5, 7, 64, 128, k=3, act=1, in_step=2),        # P5 of 10 x 14 read in place; zero padding on the sub-sampled border
]
DECONV_FORMS = [
    Form("deconv_128", 5, 7, 7, 64, 128, act=1, deconv2=True),
    Form("deconv_32", 3, 5, 7, 64, 32, act=1, deconv2=True),
    Form("deconv_20", 2, 7, 7, 64, 20, act=1, deconv2=True),            # scalar on fp16 tensors (20 % 8), 80 columns padded to 128
    Form("deconv_32_row_pitch", 3, 5, 7, 64, 32, act=1, deconv2=True, out=Layout(offset=16, gap=48, row_extra=64, tail=8)),
]
# 49 input pixels per ROI row: a 128-row tile spans rows of different classes and a -1 row
SEL_FORMS = [
    Form("selected_128", 5, 7, 7, 64, 128, act=1, deconv2=True, nc=5, sel_cid=(3, -1, 0, 4, 4)),
    Form("selected_256", 4, 7, 7, 128, 256, act=1, deconv2=True, nc=5, sel_cid=(3, -1, 0, 4)),
]
ALL_FORMS = RES_SHIFT_FORMS + SPLIT_FORMS + STRIDED_FORMS + DECONV_FORMS + SEL_FORMS


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def make_operands(f, seed=0):
    """float32 operands of a form, as the entry takes them."""
    rng = np.random.default_rng(seed + sum(ord(c) for c in f.name))
    s = f.in_step
    ops = {"x": rng.standard_normal((f.B, f.H * s, f.W * s, f.Cin)).astype(np.float32)}
    wshape = (2, 2, f.Cout, f.Cin) if f.deconv2 else (f.Cout, f.k, f.k, f.Cin)
    ops["w"] = (rng.standard_normal(wshape) / np.sqrt(f.k * f.k * f.Cin)).astype(np.float32)
    ops["scale"] = (0.5 + rng.random(f.Cout)).astype(np.float32)
    ops["shift"] = (rng.standard_normal(f.Cout) * 0.1).astype(np.float32)
    if f.res_shift >= 0:
        rh, rw = ((f.OH + 1) // 2, (f.OW + 1) // 2) if f.res_shift else (f.OH, f.OW)
        ops["res"] = rng.standard_normal((f.B, rh, rw, f.Cout)).astype(np.float32)
    if f.nc:
        ops["sel_w"] = (rng.standard_normal((f.nc, f.Cout)) * 0.1).astype(np.float32)
    return ops


def image_operands(ops, b):
    return {k: (v[b:b + 1] if k in ("x", "res") else v) for k, v in ops.items()}


def as_mode_sees(mode, ops):
    """float64 copies of the operands as the mode reads them (torch_ref of tests/test_gpu_conv_kernels.py): fp16-rounded activations,
    filters and residual in f16; fp32 activations and fp16 filters in the split modes; everything as given in f32."""
    h = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float64)
    d = lambda a: np.asarray(a, np.float64)
    act = h if mode == "f16" else d
    out = {k: d(v) for k, v in ops.items()}
    out["x"] = act(ops["x"])
    out["w"] = d(ops["w"]) if mode == "f32" else h(ops["w"])
    if "res" in ops:
        out["res"] = act(ops["res"])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the float64 definitions, one per form
# ---------------------------------------------------------------------------------------------------------------------
def ref_conv_strided(x, w, k, stride, in_step):
    """K x K 'same' convolution over the view x[:, ih * in_step, iw * in_step]: tap by tap, an input pixel outside the VIEW is zero.
    x (B, H * in_step, W * in_step, Cin), w (Cout, k, k, Cin) -> (B, OH, OW, Cout)."""
    B, Hs, Ws, _ = x.shape
    H, W, pad = Hs // in_step, Ws // in_step, k // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = np.zeros((B, OH, OW, w.shape[0]))
    for ky in range(k):
        for kx in range(k):
            ih, iw = np.arange(OH) * stride + ky - pad, np.arange(OW) * stride + kx - pad
            vh, vw = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
            patch = x[:, ih[vh] * in_step][:, :, iw[vw] * in_step]
            y[np.ix_(np.arange(B), np.flatnonzero(vh), np.flatnonzero(vw))] += patch @ w[:, ky, kx, :].T
    return y


def ref_deconv2(x, w):
    """Transposed 2 x 2 stride-2 convolution as the scatter it is: out[b, 2h + dy, 2w + dx, co] = sum_ci x[b, h, w, ci] * w[dy, dx, co, ci]."""
    B, H, W, _ = x.shape
    y = np.zeros((B, 2 * H, 2 * W, w.shape[2]))
    for dy in range(2):
        for dx in range(2):
            y[:, dy::2, dx::2] = x @ w[dy, dx].T
    return y


def ref_shifted_residual(res, OH, OW, res_shift):
    """The residual an output pixel (oh, ow) adds: res[b, oh >> res_shift, ow >> res_shift]."""
    oh, ow = np.arange(OH) >> res_shift, np.arange(OW) >> res_shift
    return res[:, oh][:, :, ow]


def ref_activate(y, act):
    if act == 1:
        return np.maximum(y, 0.0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-y))
    return y


def ref_layer(f, m):
    """The activated output image (B, rows, width, Cout) of form f on operands m (as_mode_sees): rows x width = OH x OW, 2H x 2W for deconv2."""
    y = ref_deconv2(m["x"], m["w"]) if f.deconv2 else ref_conv_strided(m["x"], m["w"], f.k, f.stride, f.in_step)
    y = y * m["scale"] + m["shift"]
    if f.res_shift >= 0:
        y = y + ref_shifted_residual(m["res"], f.OH, f.OW, f.res_shift)
    return ref_activate(y, f.act)


def ref_selected_dot(y, sel_w, cid):
    """dot[b, P] = sum_co y[b, P, co] * sel_w[cid[b], co] over the output pixels P of ROI row b (rows with cid < 0: unspecified, masked by
    the caller), and abs[b, P] = sum_co |y * w|: the magnitude the forward-error bound is stated on."""
    B, C = y.shape[0], y.shape[-1]
    wrow = sel_w[np.maximum(np.asarray(cid), 0)]                       # (B, C)
    prod = y.reshape(B, -1, C) * wrow[:, None, :]
    return prod.sum(-1), np.abs(prod).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------
# where the outputs live
# ---------------------------------------------------------------------------------------------------------------------
def layout_of(f, which):
    """The entry's numbers for output `which` ('out' | 'out2') of form f: len, offset, batch_stride, pitch, row_pitch and the image it
    holds (rows, width, cols)."""
    lay = f.out if which == "out" else f.out2
    rows, width = (2 * f.H, 2 * f.W) if f.deconv2 else (f.OH, f.OW)
    cols = f.Cout if not f.n_split else (f.n_split if which == "out" else f.Cout - f.n_split)
    pitch = cols + lay.pitch_extra
    row_pitch = width * pitch + lay.row_extra
    batch_stride = rows * row_pitch + lay.gap
    return {"len": lay.offset + f.B * batch_stride + lay.tail, "offset": lay.offset, "batch_stride": batch_stride, "pitch": pitch,
            "row_pitch": row_pitch, "rows": rows, "width": width, "cols": cols}


def addresses(lo, B):
    """Element index of (b, y, x, c) in the output buffer: offset + b * batch_stride + y * row_pitch + x * pitch + c."""
    b, y, x, c = np.ix_(np.arange(B), np.arange(lo["rows"]), np.arange(lo["width"]), np.arange(lo["cols"]))
    return lo["offset"] + b * lo["batch_stride"] + y * lo["row_pitch"] + x * lo["pitch"] + c


def place(y, lo, sentinel=SENTINEL):
    """The whole buffer a launch must leave: y's elements at their addresses, the sentinel everywhere else; and the addressed mask."""
    buf = np.full(lo["len"], sentinel, np.float64)
    mask = np.zeros(lo["len"], bool)
    a = addresses(lo, y.shape[0])
    buf[a] = y
    mask[a] = True
    return buf, mask


def split_columns(f, y):
    """{'out': columns [0, n_split) (all of them without a split), 'out2': the rest}."""
    if not f.n_split:
        return {"out": y}
    return {"out": y[..., :f.n_split], "out2": y[..., f.n_split:]}


def reference(f, mode, ops):
    """What form f must leave in mode `mode`: {'out' / 'out2': (buffer, addressed mask)} or, in the selected-class mode,
    {'dot', 'abs', 'written'}: (B, 4HW) float64 dots, their magnitudes, and which ROI rows are written."""
    m = as_mode_sees(mode, ops)
    y = ref_layer(f, m)
    if f.nc:
        dot, mag = ref_selected_dot(y, m["sel_w"], f.sel_cid)
        return {"dot": dot, "abs": mag, "written": np.asarray(f.sel_cid) >= 0}
    return {k: place(v, layout_of(f, k)) for k, v in split_columns(f, y).items()}


def selected_bound(f, mode, mag):
    """The derived forward error of the fp32 dot over Cout terms, Cout * 2^-24 * sum |y w|; f16 rounds y to fp16 first: + 2^-11 * sum |y w|."""
    return f.Cout * 2.0 ** -24 * mag + (2.0 ** -11 * mag if mode == "f16" else 0.0)
