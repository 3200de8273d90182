"""What every run-length mask entry answers to a malformed set, pinned to a recording (tests/golden/rle_entry_errors.json).

The entries share one host rule for the flat set (csrc/rle_set_host.cpp) and one staging on the device (StagedRle, csrc/api_rle_stage.h);
the recording was made from the commit before they did, so that status and the full mrcnn_last_error() text of every entry — the three
drawing entries, rle_to_polygons, rle_morph, rle_combine, rle_components, rle_components_select, rle_measure, rle_convex_hull and the
_host definition of each — stay what they were.  The set is three RLEs of planes 20x30, 7x5 and 16x16 (three images of one slot for the
per-image entries), and the table below malforms it one way at a time.  Every output is filled with the byte 0x77 first: a refusal
writes nothing, except that a capacity refusal writes what the header says it writes, and which arrays those are is recorded too.

The rows that are answered before a device is looked for — every row of the definitions, and the rows of the device entries called with
MRCNN_HOST that the recording machine answered without a GPU — run without one.  The others (device memory; host memory where the
answer comes from the device) are marked gpu.  Two corners differ from the earlier commit on purpose, listed under "changed_from_parent"
in the recording with the answer they had.  Both are null counts with run_offsets that start above 0 and hold no runs: the drawing and
polygon device entries no longer call that "null counts" (their definitions never did) and name the RLE that sums to 0; and the flat
entries in host memory (morph, combine, components, measure, hull) no longer copy from the null pointer — that row was not run on the
earlier commit and holds what device memory always answered.

`python tests/test_rle_entries_errors.py --record` adds the rows this machine can answer to the recording and changes none it holds."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rle_entry_errors.json")
HOST, DEVICE = 0, 1
ERR_HIP = 3
FILL = 0x77
MEMS = {"definition": None, "host": HOST, "device": DEVICE}


def _lib():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


def _ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def _encode(P):
    flat = np.asarray(P, np.uint8).T.reshape(-1)
    at = np.flatnonzero(np.diff(np.concatenate(([0], flat))))
    return np.diff(np.concatenate(([0], at, [flat.size]))).astype(np.uint32)


def base_set():
    runs = [_encode(p) for p in (_ellipse(20, 30, 10, 15, 6, 9), np.ones((7, 5), np.uint8), _ellipse(16, 16, 8, 8, 5, 5))]
    return {"counts": np.concatenate(runs), "offs": np.concatenate(([0], np.cumsum([len(r) for r in runs]))).astype(np.int64), "n": 3,
            "hs": np.array([20, 7, 16], np.int32), "ws": np.array([30, 5, 16], np.int32), "short": False}


def _edit(a, i, v):
    b = a.copy()
    b[i] = v
    return b


def variants():
    """name -> the malformed set"""
    S = base_set()
    o = S["offs"]
    return {
        "offsets_start_negative": dict(S, offs=_edit(o, 0, -1)),
        "offsets_decrease_at_rle_1": dict(S, offs=_edit(o, 2, o[1] - 1)),
        "rle_1_sums_to_36_of_35": dict(S, counts=_edit(S["counts"], int(o[1]), S["counts"][int(o[1])] + 1)),
        "two_wrong_sums": dict(S, hs=_edit(S["hs"], 0, 21), ws=_edit(S["ws"], 2, 15)),      # the lowest is named
        "null_counts_with_runs": dict(S, counts=None),
        "null_counts_without_runs": dict(S, counts=None, offs=np.full(4, 5, np.int64)),
        "n_is_0": dict(S, n=0),
        "side_of_0": dict(S, hs=_edit(S["hs"], 1, 0)),
        "side_of_32768": dict(S, ws=_edit(S["ws"], 2, 32768)),
        "null_offsets": dict(S, offs=None),
        "capacity_one_short": dict(S, short=True),
    }


class Memory:
    """the arrays of one call in the caller's memory space; every output filled with FILL"""

    def __init__(self, mem):
        self.dev = mem == DEVICE
        self.keep, self.outs = [], {}

    def host(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        self.keep.append(a)
        return a.ctypes.data

    def inp(self, a):
        if a is None or not self.dev:
            return self.host(a)
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def out(self, name, nbytes, on_host=False):
        if self.dev and not on_host:
            import torch
            t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
            self.outs[name] = t
            return t.data_ptr()
        a = np.full(nbytes, FILL, np.uint8)
        self.outs[name] = a
        return a.ctypes.data

    def word(self, name):
        """an int64 the entry writes in host memory in either space"""
        a = np.full(1, -9, np.int64)
        self.outs[name] = a
        return a.ctypes.data_as(C.POINTER(C.c_int64))

    def get(self, name, dtype):
        a = self.outs[name]
        return (a if isinstance(a, np.ndarray) else a.cpu().numpy()).view(dtype)

    def written(self):
        out = []
        for name, a in sorted(self.outs.items()):
            a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
            if not ((a == FILL).all() if a.dtype == np.uint8 else (a == -9).all()):
                out.append(name)
        return out


AMPLE = 4096
OUT_OFFSETS = np.array([0, 2048, 4096], np.int64)       # per image: room for 3 bytes a pixel of the largest plane


def _per_image(m, S):
    return [m.inp(S["counts"]), m.inp(S["offs"]), S["n"], 1]


def _flat(m, S):
    return [m.inp(S["counts"]), m.inp(S["offs"]), S["n"], m.host(S["hs"]), m.host(S["ws"])]


def _space(mem):
    return [] if mem is None else [mem]


def _detections(m):
    det = np.tile(np.array([0.0, 0.0, 1.0, 1.0, 1.0, 0.9], np.float32), (3, 1))
    return m.inp(det)


def rle_decode(L, S, mem, m, cap):
    f = L.mrcnn_rle_decode if mem is not None else L.mrcnn_rle_decode_host
    return f(*_per_image(m, S), m.host(S["hs"]), m.host(S["ws"]), *_space(mem), m.out("out", 6144), m.host(OUT_OFFSETS))


def instance_map_rle(L, S, mem, m, cap):
    f = L.mrcnn_instance_map_rle if mem is not None else L.mrcnn_instance_map_rle_host
    return f(_detections(m), *_per_image(m, S), m.host(S["hs"]), m.host(S["ws"]), 0.5, *_space(mem), m.out("map", 6144), m.host(OUT_OFFSETS),
             m.out("visible_areas", 12))


def render_detections_rle(L, S, mem, m, cap):
    lib = _lib()
    f = L.mrcnn_render_detections_rle if mem is not None else L.mrcnn_render_detections_rle_host
    images = (lib.Image * 3)()
    for b in range(3):
        images[b].rgb = m.inp(np.full(3 * 21 * 30, 100 + b, np.uint8))
        images[b].height, images[b].width = int(S["hs"][b]), int(S["ws"][b])
    return f(images, _detections(m), *_per_image(m, S), 0.5, 128, 2, *_space(mem), m.out("out_rgb", 6144), m.host(OUT_OFFSETS))


def rle_to_polygons(L, S, mem, m, cap):
    f = L.mrcnn_rle_to_polygons if mem is not None else L.mrcnn_rle_to_polygons_host
    vertices = AMPLE if cap is None else cap
    st = f(*_per_image(m, S), m.host(S["hs"]), m.host(S["ws"]), *_space(mem), m.out("rle_rings", 32), m.word("n_rings"), m.word("n_vertices"),
           m.out("ring_offsets", 65 * 8), m.out("ring_areas", 64 * 8), 64, m.out("xy", 8 * max(vertices, 1)), vertices)
    return st, lambda: int(m.get("n_vertices", np.int64)[0])


def _runs_out(m, cap):
    capacity = AMPLE if cap is None else cap
    return [m.out("out_counts", 4 * max(capacity, 1)), capacity, m.out("out_run_offsets", 32), m.out("areas", 12), m.out("bboxes_xywh", 48)]


def rle_morph(L, S, mem, m, cap):
    f = L.mrcnn_rle_morph if mem is not None else L.mrcnn_rle_morph_host
    st = f(*_flat(m, S), m.host(np.array([1, 2, 3], np.int32)), 0, *_space(mem), *_runs_out(m, cap))
    return st, lambda: int(m.get("out_run_offsets", np.int64)[3])


def rle_combine(L, S, mem, m, cap):
    f = L.mrcnn_rle_combine if mem is not None else L.mrcnn_rle_combine_host
    groups = 0 if S["n"] == 0 else 3                             # every RLE a group of its own: the planes differ in size
    st = f(*_flat(m, S), m.host(np.arange(4, dtype=np.int64)), m.host(np.arange(3, dtype=np.int64)), groups, 0, *_space(mem), *_runs_out(m, cap))
    return st, lambda: int(m.get("out_run_offsets", np.int64)[3])


def rle_components(L, S, mem, m, cap):
    f = L.mrcnn_rle_components if mem is not None else L.mrcnn_rle_components_host
    comps = 64 if cap is None else cap
    st = f(*_flat(m, S), 8, 1, *_space(mem), m.out("comp_offsets", 32), m.out("comp_areas", 4 * max(comps, 1)), m.out("comp_bboxes_xywh", 16 * max(comps, 1)),
           m.out("comp_flags", max(comps, 1)), comps)
    return st, lambda: int(m.get("comp_offsets", np.int64)[3])


def rle_components_select(L, S, mem, m, cap):
    f = L.mrcnn_rle_components_select if mem is not None else L.mrcnn_rle_components_select_host
    n_comps = 0 if S["n"] == 0 else 3                            # one component per plane; MERGE keeps them all
    st = f(*_flat(m, S), 8, 1, m.inp(np.ones(3, np.uint8)), n_comps, 0, *_space(mem), *_runs_out(m, cap), m.out("out_parent", 24), m.word("out_n"))
    return st, lambda: int(m.get("out_run_offsets", np.int64)[3])


def rle_measure(L, S, mem, m, cap):
    f = L.mrcnn_rle_measure if mem is not None else L.mrcnn_rle_measure_host
    return f(*_flat(m, S), *_space(mem), m.out("measures", 3 * 64 * 8))


def rle_convex_hull(L, S, mem, m, cap):
    f = L.mrcnn_rle_convex_hull if mem is not None else L.mrcnn_rle_convex_hull_host
    vertices = AMPLE if cap is None else cap
    st = f(*_flat(m, S), *_space(mem), m.out("hull_offsets", 32), m.out("hull_areas2", 24), m.out("obb", 3 * 16 * 8), m.out("xy", 8 * max(vertices, 1)),
           m.word("n_vertices"), vertices)
    return st, lambda: int(m.get("n_vertices", np.int64)[0])


ENTRIES = {f.__name__: f for f in (rle_decode, instance_map_rle, render_detections_rle, rle_to_polygons, rle_morph, rle_combine, rle_components,
                                   rle_components_select, rle_measure, rle_convex_hull)}


def answer(entry, mem_name, S):
    """{"status", "error", "written"} of one call, or None where the variant does not apply (a capacity the entry does not take)"""
    L = _lib().lib()
    mem = MEMS[mem_name]
    cap = None
    if S["short"]:                                               # what the whole set needs, by the definition
        m = Memory(None)
        got = ENTRIES[entry](L, dict(S, short=False), None, m, None)
        if not isinstance(got, tuple):
            return None
        assert got[0] == 0, L.mrcnn_last_error().decode()
        cap = got[1]() - 1
    m = Memory(mem)
    got = ENTRIES[entry](L, S, mem, m, cap)
    st = got[0] if isinstance(got, tuple) else got
    return {"status": int(st), "error": L.mrcnn_last_error().decode() if st != 0 else "", "written": m.written()}


def rows(on_gpu):
    rec = json.load(open(GOLDEN))["answers"]
    return sorted(k for k, v in rec.items() if v["gpu"] == on_gpu)


def check(key):
    rec = json.load(open(GOLDEN))["answers"][key]
    entry, mem_name, variant = key.split("/")
    got = answer(entry, mem_name, variants()[variant])
    want = {k: rec[k] for k in ("status", "error", "written")}
    assert got == want, key
    if got["status"] != 0 and variant != "capacity_one_short":
        assert got["written"] == [], key                         # a refusal leaves every output as it was


def test_the_recording_holds_every_entry_and_variant():
    rec = json.load(open(GOLDEN))
    answers = rec["answers"]
    for entry in ENTRIES:
        takes_capacity = entry not in ("rle_decode", "instance_map_rle", "render_detections_rle", "rle_measure")
        for mem_name in MEMS:
            for variant in variants():
                if variant == "capacity_one_short" and not takes_capacity:
                    continue
                assert f"{entry}/{mem_name}/{variant}" in answers, (entry, mem_name, variant)
    assert all(not v["gpu"] for k, v in answers.items() if k.split("/")[1] == "definition")
    assert all(v["gpu"] for k, v in answers.items() if k.split("/")[1] == "device")
    assert set(rec["changed_from_parent"]) <= set(answers)
    for key in rec["changed_from_parent"]:                       # the two corners, nothing else
        entry, mem_name, variant = key.split("/")
        assert variant == "null_counts_without_runs" and mem_name != "definition"
        per_image = entry in ("rle_decode", "instance_map_rle", "render_detections_rle", "rle_to_polygons")
        assert (rec["changed_from_parent"][key] is None) == (not per_image and mem_name == "host")


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_answers_without_a_device(entry):
    """the definitions, and the device entries in host memory wherever no device is needed to answer"""
    mine = [k for k in rows(False) if k.split("/")[0] == entry]
    assert len(mine) >= len(variants()) - 1
    for key in mine:
        check(key)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_answers_on_the_device(entry):
    """device memory, and host memory where the device finds the answer: the offsets read back, the wrong sums, the capacity"""
    mine = [k for k in rows(True) if k.split("/")[0] == entry]
    assert any(k.split("/")[1] == "device" for k in mine)
    for key in mine:
        check(key)


def record(skip=()):
    """adds the rows this machine can answer: with no GPU, those that need none; with one, the rest"""
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.setdefault("MRCNN_TEST_KNOBS", "1")
    import torch
    has_gpu = torch.cuda.is_available()
    rec = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"answers": {}, "changed_from_parent": {}}
    for entry in ENTRIES:
        for mem_name in MEMS:
            for variant, S in variants().items():
                key = f"{entry}/{mem_name}/{variant}"
                if key in rec["answers"] or key in skip or (mem_name == "device" and not has_gpu):
                    continue
                got = answer(entry, mem_name, S)
                if got is None or (not has_gpu and got["status"] == ERR_HIP):
                    continue
                rec["answers"][key] = dict(got, gpu=has_gpu)
                print(key, got)
    json.dump(rec, open(GOLDEN, "w"), indent=1, sort_keys=True)
    open(GOLDEN, "a").write("\n")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record(skip=[a for a in sys.argv[2:]])
