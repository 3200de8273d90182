"""The JPEG entries of this tree against the PARENT commit's, both entropy stages, in one process on the GPU.

  jpeg_entropy_ab.py --parent-lib PATH/libmaskrcnn_hip.so [--steps 20] [--warmup 3] [--seed 3] [--no-model] [--out profiles/NAME.json]

--parent-lib is the library built from the parent commit in a scratch worktree (git worktree add, make -C mask-rcnn-coreml_amd/csrc);
it is loaded beside this tree's library, and BOTH are called through ctypes into buffers allocated once, so every leg pays the same
route.  A parent from before the opt-in device stage (no mrcnn_jpeg_decode_batch_on) has no device legs.
The workload is tools/jpeg_ab.py's: eight 640x480 4:2:0 quality-90 files.  Legs alternate inside every step:

  decode_batch    parent host | this tree host | parent device | this tree device       each ending in a device synchronise
  predict_jpegs   the same four, batch 8 on the full-size artefact bench.py builds, results left on the device
Outputs are compared bit for bit with the parent's host leg before anything is timed.
Also reported: the bytes uploaded per batch both ways, the rounds to convergence (mrcnn_jpeg_coefficients' stats) and the stage times of
mrcnn_jpeg_last_stage_ms — with the device stage its host_ms runs from the headers to the verdict words (marker scan, upload, the
entropy launches and their synchronise), device_ms is the inverse DCT and the colour conversion as before.
Every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it.  `verdict` holds, per pair of
legs, both medians, both spreads (max - min) / median, and `pass`: this tree's median is no more than the parent's median times one
plus the parent leg's own spread in this run.  The exit status is 1 if a pair does not pass."""
import argparse, ctypes as C, importlib, json, os, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")
HOST, DEVICE = 0, 1


def bind(lib, L):
    vp = C.c_void_p
    lib.mrcnn_last_error.restype = C.c_char_p
    lib.mrcnn_jpeg_last_stage_ms.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mrcnn_model_load.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    lib.mrcnn_jpeg_decode_batch.argtypes = [C.POINTER(L.Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    lib.mrcnn_maskrcnn_predict_jpegs.argtypes = [vp, C.POINTER(L.Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    if hasattr(lib, "mrcnn_jpeg_decode_batch_on"):
        lib.mrcnn_jpeg_decode_batch_on.argtypes = [C.POINTER(L.Jpeg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        lib.mrcnn_maskrcnn_predict_jpegs_on.argtypes = [vp, C.POINTER(L.Jpeg), C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    return lib


def run_legs(legs, steps, warmup, sync, after=None):
    """Alternates the legs inside every step; {leg: [seconds]} of the timed steps."""
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            sync()
            dt = time.perf_counter() - t0
            if step >= warmup:
                times[k].append(dt)
                if after:
                    after(k)
    return times


def verdict(stats):
    """Per stage (host, device): this tree's leg against the parent's."""
    out = {}
    for stage in ("host", "device"):
        if "parent_" + stage not in stats:
            continue
        p, t = stats["parent_" + stage]["ms"], stats[stage]["ms"]
        spread_p, spread_t = (p["max"] - p["min"]) / p["median"], (t["max"] - t["min"]) / t["median"]
        out[stage] = {"parent_median_ms": p["median"], "median_ms": t["median"], "parent_spread": spread_p, "spread": spread_t,
                      "pass": t["median"] <= p["median"] * (1 + spread_p)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import jpeg_ab
    assert torch.cuda.is_available(), "jpeg_entropy_ab.py measures on the GPU: there is no fallback"
    J = importlib.import_module("mask-rcnn-coreml_amd.jpeg")
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    libs = {"parent_": bind(C.CDLL(os.path.abspath(args.parent_lib)), L), "": bind(C.CDLL(L.SO_PATH), L)}
    assert os.path.realpath(args.parent_lib) != os.path.realpath(L.SO_PATH), "--parent-lib is this tree's own library"
    stages = {"host": HOST, "device": DEVICE}
    names = [p + s for s in stages for p in libs if s == "host" or hasattr(libs[p], "mrcnn_jpeg_decode_batch_on")]
    files, what, _ = jpeg_ab.make_files(args.seed)
    B = len(files)
    res = {"git_head": jpeg_ab.git_head(), "parent_lib": args.parent_lib, "workload": what, "file_bytes": [len(f) for f in files], "steps": args.steps,
           "warmup": args.warmup, "legs": names}
    table, keep = J.file_table(files)
    sizes = [(J.info(f)["height"], J.info(f)["width"]) for f in files]
    offsets = np.zeros(B, np.int64)
    total = 0
    for b, (h, w) in enumerate(sizes):
        offsets[b] = total
        total += (h * w * 3 + 15) // 16 * 16
    hs, ws = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rgb = {k: torch.zeros(total, dtype=torch.uint8, device="cuda") for k in names}

    def decode(k):
        lib, stage = libs["parent_" if k.startswith("parent_") else ""], stages[k.split("_")[-1]]
        tail = (rgb[k].data_ptr(), offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data)
        st = lib.mrcnn_jpeg_decode_batch(table, B, L.DEVICE, *tail) if stage == HOST else lib.mrcnn_jpeg_decode_batch_on(table, B, L.DEVICE, stage, *tail)
        assert st == 0, lib.mrcnn_last_error()

    # equality first, and what the two paths upload
    for k in names:
        decode(k)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(rgb[k], rgb["parent_host"]), k
    coef, block0, st_dev = J.coefficients(files, 1)
    want, _, _ = J.coefficients(files, 0)
    assert np.array_equal(coef, want) and list(st_dev[:2]) == [B, 0], st_dev.tolist()
    res["device_entropy"] = {"files_clean": int(st_dev[0]), "files_fell_back": int(st_dev[1]), "most_rounds_of_a_workgroup": int(st_dev[2]), "units": int(st_dev[3])}
    # (exact: the coefficient array, and the files' bytes; the device path adds its tables and plan, a few KB per file)
    res["upload_bytes_per_batch"] = {"host_entropy_coefficients": int(block0[B]) * 128, "device_entropy_file_bytes": int(sum(len(f) for f in files))}

    stage_ms = {k: ([], []) for k in names}
    h, d = C.c_float(0), C.c_float(0)

    def stage_of(k):
        lib = libs["parent_" if k.startswith("parent_") else ""]
        assert lib.mrcnn_jpeg_last_stage_ms(C.byref(h), C.byref(d)) == 0
        stage_ms[k][0].append(h.value * 1e-3); stage_ms[k][1].append(d.value * 1e-3)

    times = run_legs({k: (lambda k=k: decode(k)) for k in names}, args.steps, args.warmup, torch.cuda.synchronize, stage_of)
    res["decode_batch"] = {k: jpeg_ab.stats(v, B) for k, v in times.items()}
    res["decode_batch_stage_ms"] = {k: {"host_ms": jpeg_ab.stats(v[0], B)["ms"], "device_ms": jpeg_ab.stats(v[1], B)["ms"]} for k, v in stage_ms.items()}
    res["decode_batch_verdict"] = verdict(res["decode_batch"])

    if args.out:                     # (the decode legs are on file even if the model legs cannot run)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not args.no_model:
        pkg = importlib.import_module("mask-rcnn-coreml_amd")
        models = importlib.import_module("mask-rcnn-coreml_amd.models")
        weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
        convert = importlib.import_module("mask-rcnn-coreml_amd.convert")
        cfg = pkg.ModelConfig(architecture="resnet101", input_image_shape=(1024, 1024, 3), num_classes=81, pre_nms_max_proposals=6000)
        mdir = tempfile.mkdtemp(prefix="mrcnn_jpeg_")
        weights.save_synthetic_models(mdir, cfg, seed=0, forced_load=True)
        convert.calibrate_artefact(mdir, np.random.default_rng(7).integers(0, 256, (2, 1024, 1024, 3), dtype=np.uint8), verbose=False)
        m = models.load_maskrcnn(mdir, max_batch=B)              # (for the output shapes)
        handles = {}
        for p, lib in libs.items():
            for setter, name in (("mrcnn_config_set_anchors_path", "anchors.bin"), ("mrcnn_config_set_classifier_path", "Classifier.mrcw"),
                                 ("mrcnn_config_set_mask_path", "Mask.mrcw")):
                getattr(lib, setter).argtypes = [C.c_char_p]
                assert getattr(lib, setter)(os.path.join(mdir, name).encode()) == 0, lib.mrcnn_last_error()
            handles[p] = C.c_void_p()
            st = lib.mrcnn_model_load(L.MODEL_MASKRCNN, os.path.join(mdir, "MaskRCNN.mrcw").encode(), B, L.DEFAULT, C.byref(handles[p]))
            assert st == 0, lib.mrcnn_last_error()
        det = {k: torch.zeros((B, m.max_detections, 6), dtype=torch.float32, device="cuda") for k in names}
        mask = {k: torch.zeros((B, m.max_detections, m.mask_size, m.mask_size), dtype=torch.float32, device="cuda") for k in names}
        del m

        def predict(k):
            p = "parent_" if k.startswith("parent_") else ""
            lib, stage = libs[p], stages[k.split("_")[-1]]
            tail = (det[k].data_ptr(), mask[k].data_ptr(), hs.ctypes.data, ws.ctypes.data)
            st = (lib.mrcnn_maskrcnn_predict_jpegs(handles[p], table, B, L.DEVICE, *tail) if stage == HOST else
                  lib.mrcnn_maskrcnn_predict_jpegs_on(handles[p], table, B, L.DEVICE, stage, *tail))
            assert st == 0, lib.mrcnn_last_error()

        for k in names:
            predict(k)
        torch.cuda.synchronize()
        for k in names:
            assert torch.equal(det[k], det["parent_host"]) and torch.equal(mask[k], mask["parent_host"]), f"predict_jpegs: {k} differs from the parent's host leg"
        ptimes = run_legs({k: (lambda k=k: predict(k)) for k in names}, args.steps, args.warmup, torch.cuda.synchronize)
        res["predict_jpegs"] = {k: jpeg_ab.stats(v, B) for k, v in ptimes.items()}
        res["predict_jpegs_verdict"] = verdict(res["predict_jpegs"])
    del keep
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ok = all(v["pass"] for key in ("decode_batch_verdict", "predict_jpegs_verdict") for v in res.get(key, {}).values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
