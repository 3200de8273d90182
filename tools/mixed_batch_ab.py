#!/usr/bin/env python
"""What a mixed-size batch buys a host, and what the ragged paste kernel costs.

  mixed_batch_ab.py [--modes f32x3,f16] [--steps 20] [--warmup 5] [--out profiles/mixed_batch_ab.json]
      Full-size artefact as bench.py builds it (R101+FPN 1024², f32x3 calibrated through convert.calibrate_artefact; f16), eight HOST
      images of eight COCO-like sizes.  Per step, interleaved in one process:
        A  eight predict_scalefit calls of batch 1       (all a host could do before predict_images existed)
        B  one predict_images call of batch 8
        C  predict_scalefit batch 8 on eight images of ONE size with the same total pixel count   (the existing path: the ceiling)
      images/s of each with the per-step spread (min / median / max of the step times) go to the JSON file.
  mixed_batch_ab.py --paste [--repeats 5]
      Only launches: mrcnn_paste_masks_source on batch 8 x 100 rows at the eight sizes, then — on the sizes whose width is a
      multiple of 4 — the same kernel against mrcnn_paste_masks (one launch per image), device buffers.  Run it under
      `rocprofv3 --kernel-trace --stats -d DIR -- python tools/mixed_batch_ab.py --paste`, then
  mixed_batch_ab.py --digest DIR [--out ...]
      reads the kernel trace and adds µs and bytes written / µs of both kernels to the JSON file."""
import argparse, csv, ctypes as C, glob, importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (768, 1024), (612, 612), (720, 1280)]      # (h, w)
ROWS = 100


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def spread(ts, images):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"images_per_s": images / med, "step_ms": {"min": ts[0] * 1e3, "median": med * 1e3, "max": ts[-1] * 1e3},
            "images_per_s_range": [images / ts[-1], images / ts[0]]}


def run_ab(args):
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    convert = importlib.import_module("mask-rcnn-coreml_amd.convert")
    cfg = pkg.ModelConfig(architecture="resnet101", input_image_shape=(1024, 1024, 3), num_classes=81, pre_nms_max_proposals=6000)
    d = tempfile.mkdtemp(prefix="mrcnn_mixed_")
    weights.save_synthetic_models(d, cfg, seed=0, forced_load=True)
    rng = np.random.default_rng(1)
    mixed = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    pixels = sum(h * w for h, w in SIZES) // len(SIZES)
    w1 = int(round((pixels * 4 / 3) ** 0.5)); h1 = pixels // w1                 # one 4:3 size with the same pixel count per image
    same = rng.integers(0, 256, (len(SIZES), h1, w1, 3), dtype=np.uint8)
    result = {"git_head": git_head(), "sizes_hw": SIZES, "one_size_hw": [h1, w1], "steps": args.steps, "warmup": args.warmup, "modes": {}}
    for mode in args.modes.split(","):
        if mode == "f32x3":
            calib = np.random.default_rng(7).integers(0, 256, (2, 1024, 1024, 3), dtype=np.uint8)
            convert.calibrate_artefact(d, calib, verbose=False)
            m = models.load_maskrcnn(d, max_batch=len(SIZES))
            assert m.compute_dtype == "f32x3", m.compute_dtype
        else:
            m = models.load_maskrcnn(d, max_batch=len(SIZES), compute_dtype=mode)
        legs = {"A": lambda: [m.predict_scalefit(im[None]) for im in mixed], "B": lambda: m.predict_images(mixed), "C": lambda: m.predict_scalefit(same)}
        times = {k: [] for k in legs}
        r0 = m.get_int("range_recoveries")
        for step in range(args.warmup + args.steps):
            for k, leg in legs.items():
                t0 = time.perf_counter()
                leg()
                if step >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        rec = {k: spread(v, len(SIZES)) for k, v in times.items()}
        rec["B_over_A"] = rec["B"]["images_per_s"] / rec["A"]["images_per_s"]
        rec["C_spread_images_per_s"] = rec["C"]["images_per_s_range"][1] - rec["C"]["images_per_s_range"][0]
        rec["B_within_C_spread"] = bool(rec["B"]["images_per_s"] >= rec["C"]["images_per_s"] - rec["C_spread_images_per_s"])
        rec["range_recoveries_during_run"] = m.get_int("range_recoveries") - r0
        result["modes"][mode] = rec
        print(mode, json.dumps(rec), flush=True)
        del m
    merge(args.out, result)


def merge(path, update):
    cur = {}
    if os.path.exists(path):
        cur = json.load(open(path))
    cur.update(update)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(cur, open(path, "w"), indent=1)
    print(json.dumps(update))


def synthetic_records(batch, rng):
    det = np.zeros((batch, ROWS, 6), np.float32)
    y1 = rng.random((batch, ROWS)) * 0.6 + 0.1; x1 = rng.random((batch, ROWS)) * 0.6 + 0.1
    det[..., 0], det[..., 1] = y1, x1
    det[..., 2] = np.minimum(0.95, y1 + 0.02 + rng.random((batch, ROWS)) * 0.4); det[..., 3] = np.minimum(0.95, x1 + 0.02 + rng.random((batch, ROWS)) * 0.4)
    det[..., 4] = rng.integers(1, 80, (batch, ROWS)); det[..., 5] = 0.7 + 0.3 * rng.random((batch, ROWS))
    return det, rng.random((batch, ROWS, 28, 28)).astype(np.float32)


def run_paste(args):
    import torch
    lib = importlib.import_module("mask-rcnn-coreml_amd._lib")
    L = lib.lib()
    rng = np.random.default_rng(5)

    def source(sizes):
        det, masks = synthetic_records(len(sizes), rng)
        hs = np.array([s[0] for s in sizes], np.int32); ws = np.array([s[1] for s in sizes], np.int32)
        nbytes = ROWS * hs.astype(np.int64) * ws
        padded = (nbytes + 15) // 16 * 16
        offs = np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64)
        det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
        src_g = torch.empty_like(det_g)
        out = torch.empty(int(padded.sum()), dtype=torch.uint8, device="cuda")
        for _ in range(args.repeats + 1):                                   # (the first launch of each kind is the warm-up)
            lib.check(L.mrcnn_paste_masks_source(det_g.data_ptr(), masks_g.data_ptr(), len(sizes), ROWS, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024,
                                                 C.c_float(0.5), lib.DEVICE, src_g.data_ptr(), out.data_ptr(), offs.ctypes.data))
        return src_g, masks_g, out
    source(SIZES)                                                           # the eight sizes: 8 x 100 rows
    aligned = [s for s in SIZES if s[1] % 4 == 0]
    src_g, masks_g, out = source(aligned)                                   # the same kernel on the sizes the old entry accepts ...
    for _ in range(args.repeats + 1):                                       # ... and the old entry on the same boxes, one launch per image
        for b, (h, w) in enumerate(aligned):
            lib.check(L.mrcnn_paste_masks(src_g[b].data_ptr(), 6, masks_g[b].data_ptr(), ROWS, 28, h, w, C.c_float(0.5), lib.DEVICE, out.data_ptr()))
    torch.cuda.synchronize()


def run_digest(args):
    rows = []
    for f in glob.glob(os.path.join(args.digest, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    ragged = [us(r) for r in rows if "k_paste_masks_ragged" in r["Kernel_Name"]]
    unlb = [us(r) for r in rows if "k_unletterbox_boxes" in r["Kernel_Name"]]
    old = [us(r) for r in rows if "k_paste_masks" in r["Kernel_Name"] and "ragged" not in r["Kernel_Name"]]
    n = (len(ragged) // 2) - 1                                              # repeats per kind (after one warm-up launch each)
    aligned = [s for s in SIZES if s[1] % 4 == 0]
    bytes_all = ROWS * sum(h * w for h, w in SIZES); bytes_al = ROWS * sum(h * w for h, w in aligned)
    all8 = ragged[1:n + 1]; al = ragged[n + 2:]
    per = len(aligned)
    old_rep = [sum(old[(i + 1) * per:(i + 2) * per]) for i in range(n)]     # (repeat 0 is the warm-up)
    rate = lambda b, ts: [b / t for t in ts]
    rec = {"git_head": git_head(), "paste": {
        "rows": ROWS, "repeats": n,
        "ragged_all_sizes": {"bytes": bytes_all, "us": all8, "bytes_per_us": rate(bytes_all, all8)},
        "ragged_aligned_sizes": {"sizes_hw": aligned, "bytes": bytes_al, "us": al, "bytes_per_us": rate(bytes_al, al)},
        "k_paste_masks_aligned_sizes": {"launches_per_repeat": per, "bytes": bytes_al, "us": old_rep, "bytes_per_us": rate(bytes_al, old_rep)},
        "k_unletterbox_boxes_us": unlb}}
    p = rec["paste"]
    o = p["k_paste_masks_aligned_sizes"]["bytes_per_us"]
    p["k_paste_masks_spread_bytes_per_us"] = max(o) - min(o)
    med = lambda v: sorted(v)[len(v) // 2]
    p["ragged_not_below_old_minus_spread"] = bool(med(p["ragged_aligned_sizes"]["bytes_per_us"]) >= med(o) - p["k_paste_masks_spread_bytes_per_us"])
    merge(args.out, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f32x3,f16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paste", action="store_true")
    ap.add_argument("--digest", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_batch_ab.json"))
    a = ap.parse_args()
    run_digest(a) if a.digest else (run_paste(a) if a.paste else run_ab(a))
