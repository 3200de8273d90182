"""The opt-in device entropy stage (entropy="device") against the PARENT commit's entries, in one process on the GPU.

  jpeg_entropy_ab.py --parent-lib PATH/libmaskrcnn_hip.so [--steps 20] [--warmup 3] [--seed 3] [--no-model] [--out profiles/jpeg_entropy_ab.json]

--parent-lib is the library built from the parent commit in a scratch worktree (git worktree add, make -C mask-rcnn-coreml_amd/csrc);
it is loaded beside this tree's library and its mrcnn_jpeg_decode_batch / mrcnn_maskrcnn_predict_jpegs are called through ctypes.
The workload is tools/jpeg_ab.py's: eight 640x480 4:2:0 quality-90 files.  Legs alternate inside every step:

  decode_batch    parent | this tree entropy="host" | this tree entropy="device"      each ending in a device synchronise
  predict_jpegs   parent | this tree entropy="device"      batch 8 on the full-size artefact bench.py builds, results left on the device
                  and the call ended by a synchronise; detections and masks compared bit for bit before anything is timed
Also reported: the bytes uploaded per batch both ways, the rounds to convergence (mrcnn_jpeg_coefficients' stats) and the stage times of
mrcnn_jpeg_last_stage_ms — with entropy="device" its host_ms runs from the headers to the verdict words (marker scan, upload, the
entropy launches and their synchronise), device_ms is the inverse DCT and the colour conversion as before.
Every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it."""
import argparse, ctypes as C, importlib, json, os, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")


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
    P = C.CDLL(os.path.abspath(args.parent_lib))
    assert not hasattr(P, "mrcnn_jpeg_decode_batch_on"), "--parent-lib is not the parent commit's library"
    vp = C.c_void_p
    P.mrcnn_jpeg_decode_batch.argtypes = [C.POINTER(L.Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    P.mrcnn_maskrcnn_predict_jpegs.argtypes = [vp, C.POINTER(L.Jpeg), C.c_int, C.c_int, vp, vp, vp, vp]
    P.mrcnn_model_load.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    P.mrcnn_last_error.restype = C.c_char_p
    files, what, _ = jpeg_ab.make_files(args.seed)
    B = len(files)
    res = {"git_head": jpeg_ab.git_head(), "parent_lib": args.parent_lib, "workload": what, "file_bytes": [len(f) for f in files], "steps": args.steps,
           "warmup": args.warmup}
    table, keep = J.file_table(files)
    sizes = [(J.info(f)["height"], J.info(f)["width"]) for f in files]
    offsets = np.zeros(B, np.int64)
    total = 0
    for b, (h, w) in enumerate(sizes):
        offsets[b] = total
        total += (h * w * 3 + 15) // 16 * 16
    pbuf = torch.empty(total, dtype=torch.uint8, device="cuda")
    hs, ws = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def parent_decode():
        st = P.mrcnn_jpeg_decode_batch(table, B, L.DEVICE, pbuf.data_ptr(), offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data)
        assert st == 0, P.mrcnn_last_error()

    # equality first, and what the two paths upload
    parent_decode()
    torch.cuda.synchronize()
    for entropy in ("host", "device"):
        got, _ = J.decode_batch(files, device=True, entropy=entropy)
        for b, g in enumerate(got):
            o = int(offsets[b])
            assert torch.equal(g.reshape(-1), pbuf[o:o + g.numel()]), (entropy, b)
    coef, block0, st_dev = J.coefficients(files, 1)
    want, _, _ = J.coefficients(files, 0)
    assert np.array_equal(coef, want) and list(st_dev[:2]) == [B, 0], st_dev.tolist()
    res["device_entropy"] = {"files_clean": int(st_dev[0]), "files_fell_back": int(st_dev[1]), "most_rounds_of_a_workgroup": int(st_dev[2]), "units": int(st_dev[3])}
    # (exact: the coefficient array, and the files' bytes; the device path adds its tables and plan, a few KB per file)
    res["upload_bytes_per_batch"] = {"host_entropy_coefficients": int(block0[B]) * 128, "device_entropy_file_bytes": int(sum(len(f) for f in files))}

    legs = {"parent": parent_decode, "host": lambda: J.decode_batch(files, device=True, entropy="host"),
            "device": lambda: J.decode_batch(files, device=True, entropy="device")}
    times = {k: [] for k in legs}
    stage = {"host": ([], []), "device": ([], [])}
    h, d = C.c_float(0), C.c_float(0)
    for step in range(args.warmup + args.steps):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                times[k].append(dt)
                if k in stage:
                    L.check(L.lib().mrcnn_jpeg_last_stage_ms(C.byref(h), C.byref(d)))
                    stage[k][0].append(h.value * 1e-3); stage[k][1].append(d.value * 1e-3)
    res["decode_batch"] = {k: jpeg_ab.stats(v, B) for k, v in times.items()}
    res["decode_batch_stage_ms"] = {k: {"host_ms": jpeg_ab.stats(v[0], B)["ms"], "device_ms": jpeg_ab.stats(v[1], B)["ms"]} for k, v in stage.items()}
    res["decode_batch_device_over_parent"] = res["decode_batch"]["device"]["images_per_s"] / res["decode_batch"]["parent"]["images_per_s"]

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
        m = models.load_maskrcnn(mdir, max_batch=B)
        for setter, name in (("mrcnn_config_set_anchors_path", "anchors.bin"), ("mrcnn_config_set_classifier_path", "Classifier.mrcw"),
                             ("mrcnn_config_set_mask_path", "Mask.mrcw")):
            getattr(P, setter).argtypes = [C.c_char_p]
            assert getattr(P, setter)(os.path.join(mdir, name).encode()) == 0, P.mrcnn_last_error()
        handle = vp()
        st = P.mrcnn_model_load(L.MODEL_MASKRCNN, os.path.join(mdir, "MaskRCNN.mrcw").encode(), B, L.DEFAULT, C.byref(handle))
        assert st == 0, P.mrcnn_last_error()
        pdet = torch.empty((B, m.max_detections, 6), dtype=torch.float32, device="cuda")
        pmask = torch.empty((B, m.max_detections, m.mask_size, m.mask_size), dtype=torch.float32, device="cuda")

        def parent_predict():
            st = P.mrcnn_maskrcnn_predict_jpegs(handle, table, B, L.DEVICE, pdet.data_ptr(), pmask.data_ptr(), hs.ctypes.data, ws.ctypes.data)
            assert st == 0, P.mrcnn_last_error()

        parent_predict()
        torch.cuda.synchronize()
        det, mask, _ = m.predict_jpegs(files, entropy="device")
        assert torch.equal(det, pdet) and torch.equal(mask, pmask), "predict_jpegs(entropy='device') differs from the parent's predict_jpegs"
        plegs = {"parent": parent_predict, "device": lambda: m.predict_jpegs(files, entropy="device")}
        ptimes = {k: [] for k in plegs}
        for step in range(args.warmup + args.steps):
            for k, leg in plegs.items():
                t0 = time.perf_counter()
                leg()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    ptimes[k].append(dt)
        res["predict_jpegs"] = {k: jpeg_ab.stats(v, B) for k, v in ptimes.items()}
        res["predict_jpegs_device_over_parent"] = res["predict_jpegs"]["device"]["images_per_s"] / res["predict_jpegs"]["parent"]["images_per_s"]
    del keep
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
