"""The forms the Python wrappers of the run-length mask entries take and return (detection.py over _marshal.py), pinned to a recording
(tests/golden/rle_wrapper_forms.json) made from the commit before the wrappers shared one set object and one capacity retry.

The set is tiny: two images of 5 x 7 and 6 x 4 with two RLEs each, one of them empty — and the degenerate sets the normaliser treats on
their own: no image, images without RLEs, a pair whose counts are empty.  Every public rle_* wrapper, instance_map_rle and
render_detections_rle is called with the set as rows and as a (counts, run_offsets) pair.  The recording holds per call the nesting of
the result, every array's memory space, dtype, shape and a digest of its bytes — or the exception's type and text — and every
ValueError the wrappers raise themselves; each such line is kept as its digest, and a test that fails prints the line of today.

Without a GPU the _host twins run (and the ValueErrors, which are raised before the library is called).  On the GPU the wrappers
themselves run with the tiny set as numpy rows and pair, as a pair of CUDA tensors and as numpy with device="cuda": the results lie
where the recording says, have its dtypes and shapes, and equal the host definitions' values bit for bit (uint32 is int32 on the device).

`python tests/test_rle_wrapper_forms.py --record` adds the calls this machine can answer to the recording and changes none it holds."""
import hashlib
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rle_wrapper_forms.json")
HOST_FORMS = ("rows", "pair", "rows/no_image", "pair/no_image", "rows/no_slot", "pair/no_slot", "pair/empty_counts")
GPU_FORMS = ("rows", "pair", "cuda_pair", "rows@cuda", "pair@cuda")         # the tiny set; the first two go through host memory
NO_DEVICE_ARGUMENT = ("instance_map_rle", "render_detections_rle", "rle_rows_of")


def _D():
    return importlib.import_module("mask-rcnn-coreml_amd.detection")


def _encode(P):
    flat = np.asarray(P, np.uint8).T.reshape(-1)
    at = np.flatnonzero(np.diff(np.concatenate(([0], flat))))
    return np.diff(np.concatenate(([0], at, [flat.size]))).astype(np.uint32)


SIZES = [(5, 7), (6, 4)]
PLANES = [[np.array([[1, 1, 1, 0, 0, 0, 1], [1, 0, 1, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0]], np.uint8),   # a hole, specks
           np.zeros((5, 7), np.uint8)],                                                                                                           # the empty one
          [np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]], np.uint8),
           np.array([[0, 1, 1, 0], [0, 1, 1, 0], [1, 1, 1, 1], [0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.uint8)]]
DET = np.array([[[0.0, 0.0, 1.0, 1.0, 1.0, 0.9], [0.0, 0.0, 1.0, 1.0, 2.0, 0.8]],
                [[0.0, 0.0, 1.0, 1.0, 3.0, 0.7], [0.1, 0.1, 0.9, 0.9, 1.0, 0.0]]], np.float32)      # the last row is not drawn


def _rows(planes, sizes):
    return [[{"size": list(s), "counts": _encode(p)} for p in row] for row, s in zip(planes, sizes)]


def _pair(rows):
    runs = [e["counts"] for row in rows for e in row]
    counts = np.concatenate(runs) if runs else np.zeros(0, np.uint32)
    return counts.astype(np.uint32), np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64)


class Setting:
    """One way to hand the set to the wrappers: its form, the arrays' memory space and the device argument."""

    def __init__(self, form, host_definition):
        kind, _, where = form.partition("@")
        kind, _, degenerate = kind.partition("/")
        self.form, self.host_definition = form, host_definition
        self.is_pair = kind != "rows"
        self.on_device = kind == "cuda_pair" or where == "cuda"
        self.kw = {"device": "cuda"} if where == "cuda" else {}
        planes, sizes = PLANES, SIZES
        if degenerate == "no_image":
            planes, sizes = [], []
        elif degenerate == "no_slot":
            planes = [[], []]
        rows = _rows(planes, sizes)
        other = [row[::-1] for row in rows]                      # the second set of the pairwise calls: the slots of every image swapped
        self.n = sum(len(r) for r in rows)
        self.images = [np.random.default_rng(3 + b).integers(0, 256, (h, w, 3), dtype=np.uint8) for b, (h, w) in enumerate(sizes)]
        self.det = DET[:len(rows), :len(rows[0]) if rows else 0].copy() if degenerate != "no_image" else np.zeros((0, 0, 6), np.float32)
        if self.is_pair:
            self.rle, self.other, self.sizes = _pair(rows), _pair(other), list(sizes)
            if degenerate == "empty_counts":                     # two images of one RLE each, and not a run
                self.rle = self.other = (np.zeros(0, np.uint32), np.zeros(3, np.int64))
                self.n, self.det = 2, DET[:, :1].copy()
        else:
            self.rle, self.other, self.sizes = rows, other, (list(sizes) if degenerate == "no_slot" else None)
        if kind == "cuda_pair":
            self.rle, self.other = tuple(self.up(a) for a in self.rle), tuple(self.up(a) for a in self.other)
        if self.on_device:
            self.det, self.images = self.up(self.det), [self.up(im) for im in self.images]

    def up(self, a):
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()

    def f(self, name):
        """the wrapper, or its _host twin, with the device argument of this setting where it takes one"""
        fn = getattr(_D(), name + ("_host" if self.host_definition else ""))
        if self.host_definition or name in NO_DEVICE_ARGUMENT or not self.kw:
            return fn
        return lambda *a, **k: fn(*a, **k, **self.kw)

    def keep(self, of="ones"):
        """every other component kept, in the set's own memory space"""
        n_comps = len(self.f("rle_components")(self.rle, self.sizes, 4, of)[1])
        keep = (np.arange(n_comps) % 2 == 0).astype(np.uint8)
        return self.up(keep) if self.on_device else keep


IDENTITY = [0, 1, 0, 1, 1, 0, 1, 0]
GROUPS = [[0, 1], [2, 3], [3, 2, 3]]

CALLS = {
    "rle_decode_planes": lambda S: S.f("rle_decode_planes")(S.rle, S.sizes),
    "rle_to_polygons": lambda S: S.f("rle_to_polygons")(S.rle, S.sizes),
    "rle_to_polygons/nest": lambda S: S.f("rle_to_polygons")(S.rle, S.sizes, nest=True),
    "rle_to_polygons/flat": lambda S: S.f("rle_to_polygons")(S.rle, S.sizes, flat=True, tolerance=1.0, nest=True),
    "instance_map_rle": lambda S: S.f("instance_map_rle")(S.det, S.rle, S.sizes, 0.5),
    "render_detections_rle": lambda S: S.f("render_detections_rle")(S.images, S.det, S.rle, 0.5, 128, 1),
    "rle_morph/erode": lambda S: S.f("rle_morph")(S.rle, S.sizes, 1, "erode"),
    "rle_morph/per_rle": lambda S: S.f("rle_morph")(S.rle, S.sizes, [1, 0, 2, 1][:S.n], 2),
    "rle_erode": lambda S: S.f("rle_erode")(S.rle, S.sizes, [1, 0]),
    "rle_dilate": lambda S: S.f("rle_dilate")(S.rle, S.sizes, 1),
    "rle_boundary": lambda S: S.f("rle_boundary")(S.rle, S.sizes),
    "rle_boundary/radius": lambda S: S.f("rle_boundary")(S.rle, S.sizes, radius=1),
    "rle_open": lambda S: S.f("rle_open")(S.rle, S.sizes, 1),
    "rle_close": lambda S: S.f("rle_close")(S.rle, S.sizes, 1),
    "rle_components": lambda S: S.f("rle_components")(S.rle, S.sizes),
    "rle_components/zeros": lambda S: S.f("rle_components")(S.rle, S.sizes, 8, "zeros"),
    "rle_select_components/merge": lambda S: S.f("rle_select_components")(S.rle, S.sizes, S.keep()),
    "rle_select_components/zeros": lambda S: S.f("rle_select_components")(S.rle, S.sizes, S.keep("zeros"), 4, "zeros", "merge"),
    "rle_select_components/split": lambda S: S.f("rle_select_components")(S.rle, S.sizes, S.keep(), 4, "ones", "split"),
    "rle_remove_small": lambda S: S.f("rle_remove_small")(S.rle, S.sizes, 2),
    "rle_keep_largest": lambda S: S.f("rle_keep_largest")(S.rle, S.sizes),
    "rle_fill_holes": lambda S: S.f("rle_fill_holes")(S.rle, S.sizes),
    "rle_fill_holes/max_area": lambda S: S.f("rle_fill_holes")(S.rle, S.sizes, 0),
    "rle_split_components": lambda S: S.f("rle_split_components")(S.rle, S.sizes, 2),
    "rle_combine/or": lambda S: S.f("rle_combine")(S.rle, S.sizes, GROUPS, "or"),
    "rle_combine/table": lambda S: S.f("rle_combine")(S.rle, S.sizes, (np.array([0, 2, 4]), np.array([0, 1, 3, 2])), 3),
    "rle_union/groups": lambda S: S.f("rle_union")(S.rle, S.sizes, GROUPS),
    "rle_union": lambda S: S.f("rle_union")(S.rle, S.sizes, other=S.other),
    "rle_intersection": lambda S: S.f("rle_intersection")(S.rle, S.sizes, other=S.other),
    "rle_xor": lambda S: S.f("rle_xor")(S.rle, S.sizes, other=S.other),
    "rle_difference": lambda S: S.f("rle_difference")(S.rle, S.sizes, other=S.other),
    "rle_disjoint": lambda S: S.f("rle_disjoint")(S.det, S.rle, S.sizes, 0.5),
    "rle_transform": lambda S: S.f("rle_transform")(S.rle, S.sizes, IDENTITY, (4, 5)),
    "rle_transform/per_rle": lambda S: S.f("rle_transform")(S.rle, S.sizes, [IDENTITY] * S.n, [(4, 5), (3, 3), (2, 9), (4, 5)][:S.n]),
    "rle_crop": lambda S: S.f("rle_crop")(S.rle, S.sizes, (1, 1, 3, 4)),
    "rle_place": lambda S: S.f("rle_place")(S.rle, S.sizes, (1, 2), (8, 9)),
    "rle_flip": lambda S: S.f("rle_flip")(S.rle, S.sizes, True, True),
    "rle_transpose": lambda S: S.f("rle_transpose")(S.rle, S.sizes),
    "rle_rot90": lambda S: S.f("rle_rot90")(S.rle, S.sizes, 3),
    "rle_resize": lambda S: S.f("rle_resize")(S.rle, S.sizes, [(3, 5), (9, 2)]),
    "rle_resize/floor": lambda S: S.f("rle_resize")(S.rle, S.sizes, (10, 11), "floor"),
    "rle_measure": lambda S: S.f("rle_measure")(S.rle, S.sizes),
    "rle_convex_hull": lambda S: S.f("rle_convex_hull")(S.rle, S.sizes),
    "rle_convex_hull/flat": lambda S: S.f("rle_convex_hull")(S.rle, S.sizes, True),
    "rle_region_props": lambda S: S.f("rle_region_props")(S.rle, S.sizes),
}
PAIR_ONLY = {"rle_rows_of": lambda S: _D().rle_rows_of(S.rle, S.sizes)}         # (it has no _host twin: it runs under both names)


def error_calls():
    """name -> a call that the wrappers refuse themselves, before the library is asked: every one under both names"""
    rows = _rows(PLANES, SIZES)
    pair = _pair(rows)
    images = Setting("rows", True).images
    E = {}
    for twin in ("", "_host"):
        f = lambda name, twin=twin: getattr(_D(), name + twin)
        for name, call in {
            "rle_morph/op": lambda f: f("rle_morph")(rows, None, 1, "shrink"),
            "rle_morph/op_number": lambda f: f("rle_morph")(rows, None, 1, 7),
            "rle_combine/op": lambda f: f("rle_combine")(rows, None, GROUPS, "nand"),
            "rle_components/of": lambda f: f("rle_components")(rows, None, 4, "twos"),
            "rle_select_components/of": lambda f: f("rle_select_components")(rows, None, np.ones(1), 4, "twos"),
            "rle_select_components/mode": lambda f: f("rle_select_components")(rows, None, np.ones(1), 4, "ones", "cut"),
            "rle_resize/rule": lambda f: f("rle_resize")(rows, None, (3, 3), "nearest"),
            "rle_morph/three_radii": lambda f: f("rle_morph")(rows, None, [1, 2, 3], "erode"),
            "rle_erode/no_radius": lambda f: f("rle_erode")(rows, None, []),
            "rle_dilate/half_a_pixel": lambda f: f("rle_dilate")(pair, SIZES, 1.5),
            "rle_union/groups_and_other": lambda f: f("rle_union")(rows, None, GROUPS, rows),
            "rle_xor/neither": lambda f: f("rle_xor")(rows),
            "rle_difference/other_of_one_image": lambda f: f("rle_difference")(rows, None, other=rows[:1]),
            "rle_intersection/other_of_other_sizes": lambda f: f("rle_intersection")(rows, None, other=rows[::-1]),
            "rle_crop/side_of_0": lambda f: f("rle_crop")(rows, None, (0, 0, 3, 0)),
            "rle_resize/side_of_32768": lambda f: f("rle_resize")(pair, SIZES, (32768, 4)),
            "rle_crop/five_numbers": lambda f: f("rle_crop")(rows, None, (0, 0, 3, 3, 1)),
            "rle_place/half_a_pixel": lambda f: f("rle_place")(rows, None, (0.5, 0), (8, 8)),
            "instance_map_rle/det_src": lambda f: f("instance_map_rle")(DET[:, :1], rows),
            "render_detections_rle/det_src": lambda f: f("render_detections_rle")(images, DET[:1], rows),
            "rle_disjoint/det_src": lambda f: f("rle_disjoint")(DET.reshape(4, 1, 6), pair, SIZES),
            "rle_measure/rows_of_unequal_length": lambda f: f("rle_measure")([rows[0], rows[1][:1]]),
            "rle_measure/pair_without_sizes": lambda f: f("rle_measure")(pair),
            "rle_convex_hull/one_size_for_two_images": lambda f: f("rle_convex_hull")(rows, SIZES[:1]),
            "rle_region_props/sizes_swapped": lambda f: f("rle_region_props")(rows, SIZES[::-1]),
            "rle_decode_planes/three_rles_for_two_images": lambda f: f("rle_decode_planes")((pair[0], pair[1][:4]), SIZES),
            "rle_to_polygons/no_slot_without_sizes": lambda f: f("rle_to_polygons")([[], []]),
            "rle_combine/groups_of_three_tables": lambda f: f("rle_combine")(rows, None, (np.zeros(1), np.zeros(1), np.zeros(1)), "or"),
            "rle_combine/no_group_offsets": lambda f: f("rle_combine")(rows, None, (np.zeros(0), np.zeros(0)), "or"),
        }.items():
            E[f"{name}{twin and '/host'}"] = lambda call=call, f=f: call(f)
    return E


def sig(x):
    """the nesting of a result as one line; an array as space:dtype[shape]#digest of its bytes"""
    if isinstance(x, tuple):
        return "(" + ",".join(sig(v) for v in x) + ")"
    if isinstance(x, list):
        return "[" + ",".join(sig(v) for v in x) + "]"
    if isinstance(x, dict):
        return "{" + ",".join(f"{k}:{sig(v)}" for k, v in x.items()) + "}"
    if hasattr(x, "is_cuda") or isinstance(x, np.ndarray):
        where = "numpy" if isinstance(x, np.ndarray) else ("cuda" if x.is_cuda else "cpu")
        a = x if isinstance(x, np.ndarray) else x.cpu().numpy()
        return f"{where}:{a.dtype.name}{list(a.shape)}#{hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:10]}"
    if isinstance(x, np.generic):
        return f"{type(x).__name__}={x.item()!r}"
    return f"{type(x).__name__}={x!r}"


def answer(call, *args):
    try:
        return sig(call(*args))
    except Exception as e:                                       # (the type and the text are what is pinned)
        return f"raises {type(e).__name__}: {e}"


def host_answers(form):
    S = Setting(form, True)
    calls = dict(CALLS, **(PAIR_ONLY if S.is_pair else {}))
    return {("host", form, name): answer(call, S) for name, call in calls.items()}


def gpu_answers(form):
    S = Setting(form, False)
    calls = dict(CALLS, **(PAIR_ONLY if S.is_pair else {}))
    return {("gpu", form, name): answer(call, S) for name, call in calls.items()}


def error_answers():
    return {("error", "raised", name): answer(call) for name, call in error_calls().items()}


def _recording():
    return json.load(open(GOLDEN))


def _digest(line):
    return hashlib.sha1(line.encode()).hexdigest()[:10]


def _differences(got, rec):
    """the calls whose answer is not the recorded one; the recording keeps a digest of every line, so the line of today is shown"""
    return [f"{k}: recorded as {rec[k[0]][k[1]].get(k[2])}, now {_digest(v)} = {v}" for k, v in got.items() if rec[k[0]][k[1]].get(k[2]) != _digest(v)]


def test_the_recording_holds_every_call_in_every_form():
    rec = _recording()
    for space, forms in (("host", HOST_FORMS), ("gpu", GPU_FORMS)):
        assert sorted(rec[space]) == sorted(forms)
        for form in forms:
            assert sorted(rec[space][form]) == sorted(list(CALLS) + (list(PAIR_ONLY) if "pair" in form else [])), (space, form)
    assert sorted(rec["error"]["raised"]) == sorted(error_calls())


def test_the_tiny_set_is_answered_and_the_refusals_are_value_errors():
    """what the digests of the recording cannot say: no call raises on the tiny set, every refusal is a ValueError"""
    for form in ("rows", "pair"):
        assert not {k: v for k, v in host_answers(form).items() if v.startswith("raises")}
    assert not {k: v for k, v in error_answers().items() if not v.startswith("raises ValueError: ")}


@pytest.mark.parametrize("form", HOST_FORMS)
def test_the_host_twins_answer_as_recorded(form):
    bad = _differences(host_answers(form), _recording())
    assert not bad, "\n".join(bad)


def test_the_wrappers_own_refusals_are_the_recorded_ones():
    bad = _differences(error_answers(), _recording())
    assert not bad, "\n".join(bad)


def _values(line):
    """a recorded line without the memory spaces, uint32 as the device holds it"""
    return re.sub(r"\b(numpy|cuda):", "", line).replace("uint32", "int32")


@pytest.mark.gpu
@pytest.mark.parametrize("form", GPU_FORMS)
def test_the_wrappers_answer_on_the_gpu_as_recorded_and_as_the_host_twins(form):
    rec = _recording()
    got = gpu_answers(form)
    bad = _differences(got, rec)                                 # where the results lie, their dtypes and shapes: the parent's
    assert not bad, "\n".join(bad)
    host = host_answers("rows" if form.startswith("rows") else "pair")      # (pinned by the test above; they need no GPU)
    for (_, _, name), line in got.items():                       # and the values of the host definitions, bit for bit
        assert _values(line) == _values(host[("host", form.partition("@")[0].replace("cuda_", ""), name)]), name
    on_device = [k for k, v in got.items() if "cuda:" in v]
    assert bool(on_device) == (form not in ("rows", "pair")), form      # numpy in and no device named: numpy out; else tensors somewhere


def record():
    """adds the calls this machine can answer: with no GPU the host twins and the refusals, with one the wrappers on the GPU"""
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.setdefault("MRCNN_TEST_KNOBS", "1")
    import torch
    rec = _recording() if os.path.exists(GOLDEN) else {}
    for space, forms in (("host", HOST_FORMS), ("gpu", GPU_FORMS), ("error", ("raised",))):
        for form in forms:
            rec.setdefault(space, {}).setdefault(form, {})
    new = {}
    if torch.cuda.is_available():
        for form in GPU_FORMS:
            new.update(gpu_answers(form))
    else:
        for form in HOST_FORMS:
            new.update(host_answers(form))
        new.update(error_answers())
    for (space, form, name), v in new.items():
        if name not in rec[space][form]:
            rec[space][form][name] = _digest(v)
            print(space, form, name, v)
    json.dump(rec, open(GOLDEN, "w"), indent=0, sort_keys=True)
    open(GOLDEN, "a").write("\n")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
