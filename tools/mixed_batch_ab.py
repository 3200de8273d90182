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
      reads the kernel trace and adds µs and bytes written / µs of both kernels to the JSON file.
  mixed_batch_ab.py --rle [--steps 20] [--warmup 5]
      What it costs a host to GET the masks of batch 8 x 100 rows at the eight sizes, detections and masks resident on the device,
      the legs interleaved in one process after a warm-up:
        A  mrcnn_paste_masks_source on device buffers, then the copy of the planes to (pinned) host memory — transport only: the
           run-length encoding a consumer then does on the host is left out, which favours A
        B  mrcnn_masks_rle_source on device buffers, then the copy of run_offsets and of the used run lengths
      on uniform-random masks (many runs per column: the worst case for B) and, for B, on smooth blobs (what a network draws).
      min / median / max of each and the bytes each moves go to the JSON file ("rle").  Under
      `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mixed_batch_ab.py --rle`, then
  mixed_batch_ab.py --digest-rle DIR
      adds the µs of k_rle_count / k_rle_offsets / k_rle_write beside k_paste_masks_ragged's ("rle_kernels").
  mixed_batch_ab.py --score [--steps 20] [--warmup 5]
      The mask IoU of COCO scoring: batch 8 x 100 detection rows at the eight sizes against 16 synthetic ground truths per image
      (smooth blobs, rows of a second synthetic batch), everything resident on the device, legs interleaved:
        A  what the library could do before mrcnn_rle_iou: mrcnn_paste_masks_source for both sets, then the dense intersection in
           torch on the device, (d & g).sum per ground truth — the arithmetic of (d[:, None] & g[None]).sum without materialising
           the 100 x 16 x h x w intermediate, which does not fit for the larger images
        B  mrcnn_masks_rle_source for both sets, then mrcnn_rle_iou on the run-length buffers   (B_iou: mrcnn_rle_iou alone)
        M  mrcnn_coco_match on B's IoU blocks (4 categories per image, 4 area ranges x 10 thresholds) — reported, no leg to compare
      A's and B's intersections are compared once, outside the timing.  min / median / max go to the JSON file ("score").  Under
      `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mixed_batch_ab.py --score`, then
  mixed_batch_ab.py --digest-score DIR
      adds the µs of k_rle_prefix / k_rle_iou / k_coco_match ("score_kernels").
  mixed_batch_ab.py --render [--steps 20] [--warmup 5]
      What it costs to LOOK at the detections of batch 8 x 100 rows at the eight sizes (smooth blobs, every row drawn: min_score 0),
      detections, masks and source images resident on the device, the legs interleaved in one process after a warm-up:
        A_map     what the library could do before: mrcnn_paste_masks_source on device buffers, then per image the first set plane
                  per pixel in torch on the device (argmax over the planes, -1 where none is set)
        B_map     mrcnn_instance_map_source (with visible_areas)
        A_render  A_map, then the palette colour gathered per pixel and blended into the source in torch; no strokes, which favours A
        B_render  mrcnn_render_detections_source, alpha 128, stroke 3
      A's and B's maps, and A's picture and B's at stroke 0, are compared once outside the timing.  min / median / max go to the JSON
      file ("render").  Under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mixed_batch_ab.py --render`, then
  mixed_batch_ab.py --digest-render DIR
      adds the µs of k_instance_map / k_render_detections beside k_paste_masks_ragged's and their GB/s of algorithmic bytes
      ("render_kernels")."""
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


def smooth_masks(batch, rng):
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    cy = rng.uniform(8, 20, (batch, ROWS, 1, 1)); cx = rng.uniform(8, 20, (batch, ROWS, 1, 1))
    sy = rng.uniform(4, 12, (batch, ROWS, 1, 1)); sx = rng.uniform(4, 12, (batch, ROWS, 1, 1))
    return np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)).astype(np.float32)


def run_rle(args):
    import torch
    lib = importlib.import_module("mask-rcnn-coreml_amd._lib")
    L = lib.lib()
    rng = np.random.default_rng(5)
    B, n = len(SIZES), len(SIZES) * ROWS
    det, random_masks = synthetic_records(B, rng)
    hs = np.array([s[0] for s in SIZES], np.int32); ws = np.array([s[1] for s in SIZES], np.int32)
    nbytes = ROWS * hs.astype(np.int64) * ws
    padded = (nbytes + 15) // 16 * 16
    offs = np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64)
    det_g = torch.from_numpy(det).cuda()
    masks_g = {"random": torch.from_numpy(random_masks).cuda(), "smooth": torch.from_numpy(smooth_masks(B, rng)).cuda()}
    src_g = torch.empty_like(det_g)
    planes_g = torch.empty(int(padded.sum()), dtype=torch.uint8, device="cuda")
    planes_h = torch.empty(int(padded.sum()), dtype=torch.uint8).pin_memory()
    ro_g = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ro_h = torch.empty(n + 1, dtype=torch.int64).pin_memory()
    areas_g = torch.empty(n, dtype=torch.int32, device="cuda"); boxes_g = torch.empty(4 * n, dtype=torch.int32, device="cuda")
    used = {}

    def rle(kind, counts_g, capacity):
        return L.mrcnn_masks_rle_source(det_g.data_ptr(), masks_g[kind].data_ptr(), B, ROWS, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024, C.c_float(0.5),
                                        lib.DEVICE, src_g.data_ptr(), counts_g.data_ptr() if counts_g is not None else None, capacity, ro_g.data_ptr(),
                                        areas_g.data_ptr(), boxes_g.data_ptr())
    counts_g, counts_h = {}, {}
    for kind in masks_g:                                                    # the size query, once, outside the timing
        assert rle(kind, None, 0) == 4
        used[kind] = int(ro_g[n].item())
        counts_g[kind] = torch.empty(used[kind], dtype=torch.int32, device="cuda")
        counts_h[kind] = torch.empty(used[kind], dtype=torch.int32).pin_memory()

    def leg_a():
        lib.check(L.mrcnn_paste_masks_source(det_g.data_ptr(), masks_g["random"].data_ptr(), B, ROWS, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024,
                                             C.c_float(0.5), lib.DEVICE, src_g.data_ptr(), planes_g.data_ptr(), offs.ctypes.data))
        planes_h.copy_(planes_g)
        torch.cuda.synchronize()

    def leg_b(kind):
        lib.check(rle(kind, counts_g[kind], used[kind]))
        ro_h.copy_(ro_g)
        counts_h[kind].copy_(counts_g[kind])                                # (sized to the used part by the query above)
        torch.cuda.synchronize()
    legs = {"A": leg_a, "B": lambda: leg_b("random"), "B_smooth": lambda: leg_b("smooth")}
    times = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            if step >= args.warmup:
                times[k].append(time.perf_counter() - t0)

    def ms(ts):
        ts = sorted(ts)
        return {"min": ts[0] * 1e3, "median": ts[len(ts) // 2] * 1e3, "max": ts[-1] * 1e3}
    rec = {k: {"ms": ms(v)} for k, v in times.items()}
    rec["A"]["bytes_to_host"] = int(nbytes.sum())
    for k, kind in (("B", "random"), ("B_smooth", "smooth")):
        rec[k]["runs"] = used[kind]
        rec[k]["bytes_to_host"] = 4 * used[kind] + 8 * (n + 1)
    a = rec["A"]["ms"]
    rec["A_spread_ms"] = a["max"] - a["min"]
    rec["B_below_A_by_more_than_A_spread"] = bool(a["median"] - rec["B"]["ms"]["median"] > rec["A_spread_ms"])
    rec["B_smooth_below_A_by_more_than_A_spread"] = bool(a["median"] - rec["B_smooth"]["ms"]["median"] > rec["A_spread_ms"])
    merge(args.out, {"git_head": git_head(), "rle": dict(rec, rows=ROWS, sizes_hw=SIZES, steps=args.steps, warmup=args.warmup, host_memory="pinned")})


def run_score(args):
    import torch
    lib = importlib.import_module("mask-rcnn-coreml_amd._lib")
    L = lib.lib()
    rng = np.random.default_rng(7)
    B, NG = len(SIZES), 16
    hs = np.array([s[0] for s in SIZES], np.int32); ws = np.array([s[1] for s in SIZES], np.int32)

    class Set:
        def __init__(self, rows):
            global ROWS
            keep, ROWS = ROWS, rows                                          # (synthetic_records / smooth_masks size by the module's ROWS)
            det, _ = synthetic_records(B, rng)
            masks = smooth_masks(B, rng)
            ROWS = keep
            self.rows, self.n = rows, B * rows
            self.det, self.masks = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
            self.src = torch.empty_like(self.det)
            nbytes = rows * hs.astype(np.int64) * ws
            padded = (nbytes + 15) // 16 * 16
            self.offs = np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64)
            self.planes = torch.empty(int(padded.sum()), dtype=torch.uint8, device="cuda")
            self.ro = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
            self.areas = torch.empty(self.n, dtype=torch.int32, device="cuda")
            assert self.rle(None, 0) == 4                                    # the size query, outside the timing
            self.used = int(self.ro[self.n].item())
            self.counts = torch.empty(self.used, dtype=torch.int32, device="cuda")

        def rle(self, counts, capacity):
            return L.mrcnn_masks_rle_source(self.det.data_ptr(), self.masks.data_ptr(), B, self.rows, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024,
                                            C.c_float(0.5), lib.DEVICE, self.src.data_ptr(), counts.data_ptr() if counts is not None else None, capacity,
                                            self.ro.data_ptr(), self.areas.data_ptr(), None)

        def paste(self):
            lib.check(L.mrcnn_paste_masks_source(self.det.data_ptr(), self.masks.data_ptr(), B, self.rows, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024,
                                                 C.c_float(0.5), lib.DEVICE, self.src.data_ptr(), self.planes.data_ptr(), self.offs.ctypes.data))

        def image(self, b):
            h, w = SIZES[b]
            o = int(self.offs[b])
            return self.planes[o:o + self.rows * h * w].view(self.rows, h, w)
    D, G = Set(ROWS), Set(NG)
    n_pairs = B * ROWS * NG
    groups = (lib.IouGroup * B)()
    for b in range(B):
        groups[b].d0, groups[b].d1, groups[b].g0, groups[b].g1, groups[b].out_offset = b * ROWS, (b + 1) * ROWS, b * NG, (b + 1) * NG, b * ROWS * NG
    crowd = np.zeros(B * NG, np.uint8)
    inter_a = torch.empty(n_pairs, dtype=torch.int64, device="cuda")
    inter_b = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    iou_b = torch.empty(n_pairs, dtype=torch.float64, device="cuda")

    def leg_a():
        D.paste(); G.paste()
        for b in range(B):
            d, g = D.image(b), G.image(b)
            out = inter_a[b * ROWS * NG:(b + 1) * ROWS * NG].view(ROWS, NG)
            for j in range(NG):
                out[:, j] = (d & g[j]).sum((1, 2))
        torch.cuda.synchronize()

    def iou_only():
        lib.check(L.mrcnn_rle_iou(D.counts.data_ptr(), D.ro.data_ptr(), D.n, G.counts.data_ptr(), G.ro.data_ptr(), G.n, crowd.ctypes.data, groups, B,
                                  lib.DEVICE, inter_b.data_ptr(), iou_b.data_ptr(), n_pairs))

    def leg_b():
        lib.check(D.rle(D.counts, D.used)); lib.check(G.rle(G.counts, G.used))
        iou_only()
    # the match tables: per image 4 categories (class id % 4), detections by score, ground truths in row order
    det_h, gdet_h = D.det.cpu().numpy(), G.det.cpu().numpy()
    area_d, area_g = D.areas.cpu().numpy().astype(np.float64), G.areas.cpu().numpy().astype(np.float64)
    mg, dt_idx, gt_idx = [], [], []
    for b in range(B):
        for cat in range(4):
            di = [i for i in range(ROWS) if int(det_h[b, i, 4]) % 4 == cat]
            di = [di[i] for i in np.argsort([-det_h[b, i, 5] for i in di], kind="mergesort")]
            gi = [j for j in range(NG) if int(gdet_h[b, j, 4]) % 4 == cat]
            mg.append((b * ROWS * NG, NG, len(dt_idx), len(dt_idx) + len(di), len(gt_idx), len(gt_idx) + len(gi), b))
            dt_idx += [(b, i) for i in di]; gt_idx += [(b, j) for j in gi]
    marr = (lib.MatchGroup * len(mg))()
    for k, g in enumerate(mg):
        marr[k].iou_offset, marr[k].iou_stride, marr[k].dt0, marr[k].dt1, marr[k].gt0, marr[k].gt1 = g[:6]
    dti = np.array([i for _, i in dt_idx], np.int32); gti = np.array([j for _, j in gt_idx], np.int32)
    dta = np.array([area_d[b * ROWS + i] for b, i in dt_idx]); gta = np.array([area_g[b * NG + j] for b, j in gt_idx])
    gtc = np.zeros(gti.size, np.uint8)
    rngs = np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]], np.float64); thrs = np.linspace(.5, .95, 10)
    dm = torch.empty(40 * dti.size, dtype=torch.int32, device="cuda"); dg = torch.empty(40 * dti.size, dtype=torch.uint8, device="cuda")
    gm = torch.empty(40 * gti.size, dtype=torch.int32, device="cuda")

    def leg_m():
        lib.check(L.mrcnn_coco_match(iou_b.data_ptr(), n_pairs, lib.DEVICE, marr, len(mg), dti.ctypes.data, dta.ctypes.data, dti.size, gti.ctypes.data,
                                     gta.ctypes.data, gtc.ctypes.data, gti.size, rngs.ctypes.data, 4, thrs.ctypes.data, 10, dm.data_ptr(), dg.data_ptr(),
                                     gm.data_ptr()))
    legs = {"A": leg_a, "B": leg_b, "B_iou": iou_only, "M": leg_m}
    times = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            if step >= args.warmup:
                times[k].append(time.perf_counter() - t0)
    equal = bool(torch.equal(inter_a, inter_b.to(torch.int64)))

    def ms(ts):
        ts = sorted(ts)
        return {"min": ts[0] * 1e3, "median": ts[len(ts) // 2] * 1e3, "max": ts[-1] * 1e3}
    rec = {k: {"ms": ms(v)} for k, v in times.items()}
    a = rec["A"]["ms"]
    rec["A_spread_ms"] = a["max"] - a["min"]
    rec["B_below_A_by_more_than_A_spread"] = bool(a["median"] - rec["B"]["ms"]["median"] > rec["A_spread_ms"])
    rec["intersections_equal"] = equal
    rec["A"]["plane_bytes"] = int(D.planes.numel() + G.planes.numel())
    rec["B"]["run_bytes"] = 4 * (D.used + G.used)
    rec["M"]["groups"] = len(mg)
    merge(args.out, {"git_head": git_head(), "score": dict(rec, rows=ROWS, ground_truths_per_image=NG, pairs=n_pairs, sizes_hw=SIZES, steps=args.steps,
                                                           warmup=args.warmup)})


def run_render(args):
    import torch
    lib = importlib.import_module("mask-rcnn-coreml_amd._lib")
    L = lib.lib()
    rng = np.random.default_rng(9)
    B = len(SIZES)
    det, _ = synthetic_records(B, rng)
    det[..., 5] = -np.sort(-det[..., 5], axis=1)                            # rows leave the detection layer in descending score
    masks = smooth_masks(B, rng)
    hs = np.array([s[0] for s in SIZES], np.int32); ws = np.array([s[1] for s in SIZES], np.int32)
    pixels = hs.astype(np.int64) * ws

    def layout(unit):
        padded = (unit * pixels + 15) // 16 * 16
        return np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64), int(padded.sum())
    p_offs, p_total = layout(ROWS); m_offs, m_total = layout(2); r_offs, r_total = layout(3)
    det_g, masks_g = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    src_g = torch.empty_like(det_g)
    images = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in SIZES]
    table = (lib.Image * B)()
    for b, t in enumerate(images):
        table[b].rgb, table[b].height, table[b].width = t.data_ptr(), SIZES[b][0], SIZES[b][1]
    planes_g = torch.empty(p_total, dtype=torch.uint8, device="cuda")
    map_g = torch.empty(m_total // 2, dtype=torch.int16, device="cuda")
    vis_g = torch.empty(B * ROWS, dtype=torch.int32, device="cuda")
    rgb_g = torch.empty(r_total, dtype=torch.uint8, device="cuda")
    palette = torch.tensor([[255, 0, 0], [0, 0, 255], [0, 255, 0], [255, 255, 0]], dtype=torch.int32, device="cuda")
    a_maps, a_rgb = [None] * B, [None] * B

    def a_map():
        lib.check(L.mrcnn_paste_masks_source(det_g.data_ptr(), masks_g.data_ptr(), B, ROWS, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024,
                                             C.c_float(0.5), lib.DEVICE, src_g.data_ptr(), planes_g.data_ptr(), p_offs.ctypes.data))
        for b, (h, w) in enumerate(SIZES):
            p = planes_g[int(p_offs[b]):int(p_offs[b]) + ROWS * h * w].view(ROWS, h, w)
            top, idx = p.max(0)                                             # (the first of several maxima: the lowest set plane)
            a_maps[b] = torch.where(top > 0, idx, -1).to(torch.int16)

    def leg_a_map():
        a_map()
        torch.cuda.synchronize()

    def leg_a_render():
        a_map()
        for b in range(B):
            m = a_maps[b].to(torch.int64)
            col = palette[m % 4]
            s = images[b].to(torch.int32)
            a_rgb[b] = torch.where((m >= 0)[..., None], (s * 128 + col * 128 + 128) >> 8, s).to(torch.uint8)
        torch.cuda.synchronize()

    def leg_b_map():
        lib.check(L.mrcnn_instance_map_source(det_g.data_ptr(), masks_g.data_ptr(), B, ROWS, 28, hs.ctypes.data, ws.ctypes.data, 1024, 1024, C.c_float(0.5),
                                              C.c_float(0.0), lib.DEVICE, src_g.data_ptr(), map_g.data_ptr(), m_offs.ctypes.data, vis_g.data_ptr()))

    def b_render(stroke):
        lib.check(L.mrcnn_render_detections_source(table, det_g.data_ptr(), masks_g.data_ptr(), B, ROWS, 28, 1024, 1024, C.c_float(0.5), C.c_float(0.0), 128,
                                                   stroke, lib.DEVICE, src_g.data_ptr(), rgb_g.data_ptr(), r_offs.ctypes.data))
    legs = {"A_map": leg_a_map, "B_map": leg_b_map, "A_render": leg_a_render, "B_render": lambda: b_render(3)}
    times = {k: [] for k in legs}
    for step in range(args.warmup + args.steps):
        for k, leg in legs.items():
            t0 = time.perf_counter()
            leg()
            if step >= args.warmup:
                times[k].append(time.perf_counter() - t0)
    b_render(0)
    maps_equal = rgb_equal = True
    for b, (h, w) in enumerate(SIZES):
        maps_equal &= bool(torch.equal(a_maps[b], map_g[int(m_offs[b]) // 2:int(m_offs[b]) // 2 + h * w].view(h, w)))
        rgb_equal &= bool(torch.equal(a_rgb[b], rgb_g[int(r_offs[b]):int(r_offs[b]) + 3 * h * w].view(h, w, 3)))
    b_render(3)                                                             # (leave the real picture behind, and one more launch for the trace)

    def ms(ts):
        ts = sorted(ts)
        return {"min": ts[0] * 1e3, "median": ts[len(ts) // 2] * 1e3, "max": ts[-1] * 1e3}
    rec = {k: {"ms": ms(v)} for k, v in times.items()}
    for kind in ("map", "render"):
        a = rec["A_" + kind]["ms"]
        rec[f"A_{kind}_spread_ms"] = a["max"] - a["min"]
        rec[f"B_{kind}_below_A_by_more_than_A_spread"] = bool(a["median"] - rec["B_" + kind]["ms"]["median"] > a["max"] - a["min"])
    rec["maps_equal"], rec["pictures_equal_at_stroke_0"] = maps_equal, rgb_equal
    rec["A_map"]["plane_bytes"] = int(ROWS * pixels.sum())
    rec["B_map"]["bytes_written"] = int(2 * pixels.sum())
    rec["B_render"]["bytes_read_and_written"] = int(6 * pixels.sum())
    rec["visible_pixels"] = int(vis_g.sum().item())
    merge(args.out, {"git_head": git_head(), "render": dict(rec, rows=ROWS, sizes_hw=SIZES, steps=args.steps, warmup=args.warmup, masks="smooth", min_score=0.0)})


def run_digest_render(args):
    rows = []
    for f in glob.glob(os.path.join(args.digest_render, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    pixels = sum(h * w for h, w in SIZES)
    algo = {"k_paste_masks_ragged": ROWS * pixels, "k_instance_map": 2 * pixels, "k_render_detections": 6 * pixels}

    def stat(name):
        v = sorted(us(r) for r in rows if name in r["Kernel_Name"])
        if not v:
            return {"launches": 0}
        rec = {"launches": len(v), "us": {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}}
        if name in algo:
            rec["algorithmic_bytes"] = algo[name]
            rec["gb_per_s_at_median"] = algo[name] / v[len(v) // 2] / 1e3
        return rec
    merge(args.out, {"render_kernels": {k: stat(k) for k in ("k_unletterbox_boxes", "k_paste_masks_ragged", "k_instance_map", "k_render_detections")}})


def run_digest_score(args):
    rows = []
    for f in glob.glob(os.path.join(args.digest_score, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    def stat(name):
        v = sorted(us(r) for r in rows if name in r["Kernel_Name"])
        return {"launches": len(v), "us": {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}} if v else {"launches": 0}
    merge(args.out, {"score_kernels": {k: stat(k) for k in ("k_rle_prefix", "k_rle_iou", "k_coco_match")}})


def run_digest_rle(args):
    rows = []
    for f in glob.glob(os.path.join(args.digest_rle, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    def stat(name):
        v = sorted(us(r) for r in rows if name in r["Kernel_Name"])
        return {"launches": len(v), "us": {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}} if v else {"launches": 0}
    merge(args.out, {"rle_kernels": {k: stat(k) for k in ("k_unletterbox_boxes", "k_paste_masks_ragged", "k_rle_count", "k_rle_offsets", "k_rle_write")}})


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
    ap.add_argument("--rle", action="store_true")
    ap.add_argument("--digest", metavar="DIR")
    ap.add_argument("--digest-rle", metavar="DIR")
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--digest-score", metavar="DIR")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--digest-render", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_batch_ab.json"))
    a = ap.parse_args()
    if a.digest_render:
        run_digest_render(a)
    elif a.render:
        run_render(a)
    elif a.digest_score:
        run_digest_score(a)
    elif a.score:
        run_score(a)
    elif a.digest_rle:
        run_digest_rle(a)
    elif a.rle:
        run_rle(a)
    else:
        run_digest(a) if a.digest else (run_paste(a) if a.paste else run_ab(a))
