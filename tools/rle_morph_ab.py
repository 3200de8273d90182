"""Changing run-length masks: what mrcnn_rle_morph costs on device-resident runs against the route a host has without it, and what
Boundary AP costs on top of mask AP, in one process on the GPU.

  rle_morph_ab.py [--steps 20] [--warmup 3] [--host-steps 3] [--only device] [--out profiles/rle_morph_ab.json]
  rle_morph_ab.py --share profiles/rle_morph_ab_only.json <kernel_stats.csv>

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots; BOUNDARY at r = 102, Boundary IoU's radius for that image
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch); BOUNDARY at
                   r = 16
  legs    device   detection.rle_morph on the device-resident (counts, run_offsets) pair: the result stays on the device
          host     the route a host has without the entry: the runs copied down, the sequential definition there
                   (mrcnn_rle_morph_host: a plane per RLE), the result copied back to the device.  Seconds per call on the large
                   scene, so it is timed on --host-steps calls only
  score   coco_eval.score_batch on the batch scene against a resident ground truth made of its own masks, some shifted by 3 pixels:
          "segm"; "boundary" with the bands made in the call (both caches emptied before it); "boundary" with the bands cached

Before anything is timed the device result is compared with the host definition's, array by array.  Every figure is the median of the
timed calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end synchronised.  The
kernels' share of a call comes from a second run: `rocprofv3 --kernel-trace --stats --output-format csv` around `rle_morph_ab.py --only
device`, whose kernel_stats.csv `--share` divides by that run's calls and medians (kernels k_morph_*, k_rle_prefix, k_poly_scan).
No time was promised for either route; the result says which leg won and is written down as it is."""
import argparse, csv, importlib, json, os, re, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402


def share(record, stats_csv):
    """The kernels' time per call from a rocprofv3 kernel_stats.csv of an `--only device` run, per kernel and as a share of the calls' medians."""
    rec = json.load(open(record))
    calls = sum(s["device_calls"] for s in rec["scenes"].values())
    per_call_ms = sum(s["ms"]["device"]["median"] * s["device_calls"] for s in rec["scenes"].values()) / calls
    rows = list(csv.DictReader(open(stats_csv)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname"))
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    mine = {}
    for r in rows:
        m = re.search(r"k_morph_\w+|k_rle_prefix|k_poly_scan", r[name])
        if m:
            mine[m.group(0)] = mine.get(m.group(0), 0.0) + float(r[total]) * 1e-6 / calls
    out = {"calls": calls, "entry_ms_per_call": per_call_ms, "kernel_ms_per_call": sum(mine.values()), "kernel_share": sum(mine.values()) / per_call_ms,
           "kernels_ms_per_call": dict(sorted(mine.items(), key=lambda kv: -kv[1]))}
    print(json.dumps(out))
    return 0


def timed(leg, warmup, steps):
    import torch
    out = []
    for step in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leg()
        torch.cuda.synchronize()
        if step >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def score_legs(CE, CR, D, bdet, bmask, bsizes, encoded, args):
    """the cost of Boundary AP beside mask AP on the batch scene"""
    import torch
    image_ids = list(range(1, len(bsizes) + 1))
    results = CR.coco_results(image_ids, encoded[0], encoded[1], bsizes)
    anns = []
    for k, r in enumerate(results[::2]):
        plane = CR.rle_decode(r["segmentation"])
        if k % 3 == 1:
            plane = np.roll(plane, 3, 1)
        if plane.sum() == 0:
            continue
        anns.append({"id": k + 1, "image_id": r["image_id"], "category_id": r["category_id"], "iscrowd": 0, "area": float(plane.sum()), "bbox": r["bbox"],
                     "segmentation": {"size": list(plane.shape), "counts": CR.rle_to_string(CR.rle_encode(plane)["counts"])}})
    cats = sorted(set(a["category_id"] for a in anns) | set(r["category_id"] for r in results))
    gt = CE.COCOGroundTruth({"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(image_ids, bsizes)], "categories": [{"id": c} for c in cats],
                             "annotations": anns})
    resident = gt.to_device()
    batch = CE.device_detections(image_ids, torch.from_numpy(bdet).cuda(), torch.from_numpy(bmask).cuda(), bsizes, MODEL, MODEL, 0.5)

    def cold():
        resident._bands.clear(); batch._bands.clear()
        return CE.score_batch(gt, [batch], "boundary", device_gt=resident)
    legs = {"segm": lambda: CE.score_batch(gt, [batch], "segm", device_gt=resident), "boundary_bands_made": cold,
            "boundary_bands_cached": lambda: CE.score_batch(gt, [batch], "boundary", device_gt=resident)}
    ms = {k: stats(timed(leg, args.warmup, args.steps)) for k, leg in legs.items()}
    segm, band = legs["segm"](), legs["boundary_bands_cached"]()
    return {"images": len(bsizes), "detections": len(batch.records), "ground_truths": len(anns), "AP_segm": float(segm["stats"][0]), "AP_boundary": float(band["stats"][0]),
            "ms": ms, "boundary_over_segm_cached": ms["boundary_bands_cached"]["median"] / ms["segm"]["median"],
            "boundary_over_segm_made": ms["boundary_bands_made"]["median"] / ms["segm"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--only", choices=("device",), default=None)
    ap.add_argument("--share", nargs=2, metavar=("RECORD", "KERNEL_STATS_CSV"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_morph_ab.json"))
    args = ap.parse_args()
    if args.share:
        return share(*args.share)
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    CE = importlib.import_module("mask-rcnn-coreml_amd.coco_eval")
    CR = importlib.import_module("mask-rcnn-coreml_amd.coco_results")

    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
    odet, omask, _n_objects = objects_scene(tiles, 100)
    united = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    bdet, bmask, bsizes = batch_scene()
    encoded = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
    scenes = {"tiled": (united[3], [(H_IMG, W_IMG)]), "batch": (encoded[1], bsizes)}
    rec = {"git": git_head(), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "only": args.only, "scenes": {}}
    ok = True
    for name, (rles, sizes) in scenes.items():
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())
        radius = D.boundary_radius(*sizes[0])
        torch.cuda.synchronize()

        def device():
            return D.rle_morph(pair, sizes, radius, "boundary")

        def host():
            down = (pair[0].cpu().numpy().view(np.uint32), pair[1].cpu().numpy())
            (c, o), areas, boxes = D.rle_morph_host(down, sizes, radius, "boundary")
            return (torch.from_numpy(c.view(np.int32)).cuda(), torch.from_numpy(o).cuda()), areas, boxes
        got = device()
        same = None
        if not args.only:
            want = host()
            same = bool(np.array_equal(got[0][0].cpu().numpy(), want[0][0].cpu().numpy()) and np.array_equal(got[0][1].cpu().numpy(), want[0][1].cpu().numpy())
                        and np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1]) and np.array_equal(got[2].cpu().numpy(), want[2]))
            ok = ok and same
        ms = {"device": stats(timed(device, args.warmup, args.steps))}
        if not args.only:
            ms["host"] = stats(timed(host, 1, args.host_steps))
        areas = got[1].cpu().numpy().view(np.uint32)
        scene = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "radius": radius, "op": "boundary", "runs_in": int(counts.size),
                 "runs_out": int(got[0][0].shape[0]), "masks_set": int((np.diff(offs) > 1).sum()), "band_pixels": int(areas.astype(np.int64).sum()),
                 "plane_bytes_a_host_decodes": int(sum(h * w for h, w in sizes) * len(rles[0])), "arrays_equal": same,
                 "device_calls": 1 + args.warmup + args.steps, "ms": ms}
        if not args.only:
            scene["host_over_device"] = ms["host"]["median"] / ms["device"]["median"]
        rec["scenes"][name] = scene
    if not args.only:
        rec["score"] = score_legs(CE, CR, D, bdet, bmask, bsizes, encoded, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
