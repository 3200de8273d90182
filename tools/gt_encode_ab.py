"""Polygon ground truth to RLE: the host path against the device path, in one process, on a synthetic annotation set.

  gt_encode_ab.py [--images 3000] [--seed 3] [--warmup 1] [--repeats 3] [--score] [--out profiles/gt_encode_ab.txt]

The set (seeded, no dataset ships here) has COCO-val proportions: `--images` images of the eight sizes of tools/mixed_batch_ab.py,
1-14 polygon annotations each (7.4 on average, 1-3 polygons per annotation), outlines of 12-300 vertices around objects from a few
pixels to most of the image.
    A   the path before mrcnn_rle_from_polygons_batch: COCOGroundTruth.counts() over every annotation — two ctypes calls of the host
        entry mrcnn_rle_from_polygons per annotation, one host thread
    B   COCOGroundTruth.to_device(): the whole file in one call of mrcnn_rle_from_polygons_batch, resident on the device afterwards
Both legs start from a freshly parsed COCOGroundTruth (the parse is outside the window) and are compared bit for bit before anything is
timed; B's window ends in a device synchronise.  The legs alternate, after `--warmup` untimed rounds; min / median / max of `--repeats`.
With --score, score_batch (segm) over detection batches of 8 images x 100 rows that stay on the device, against the same file, with and
without the resident ground truth (the ground truth's run lengths are then concatenated on the host and uploaded per batch); both give
the same twelve numbers, which is checked."""
import argparse, importlib, os, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(480, 640), (640, 480), (427, 640), (375, 500), (500, 333), (768, 1024), (612, 612), (720, 1280)]      # (h, w)


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def synthetic_annotations(n_images, seed):
    rng = np.random.default_rng(seed)
    images, anns = [], []
    aid = 1
    for i in range(n_images):
        h, w = SIZES[i % len(SIZES)]
        images.append({"id": i + 1, "height": h, "width": w})
        for _ in range(int(np.clip(rng.poisson(7.4), 1, 14))):
            size = float(np.exp(rng.uniform(np.log(6.0), np.log(0.45 * min(h, w)))))          # the object's radius: log-uniform
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            polys = []
            for p in range(int(rng.choice([1, 1, 1, 2, 3]))):
                k = int(np.clip(12 + size * rng.uniform(0.3, 1.2), 12, 300))
                ang = np.sort(rng.uniform(0, 2 * np.pi, k))
                rr = size * (0.6 + 0.4 * rng.random(k)) * (1.0 if p == 0 else 0.4)
                ox, oy = (0.0, 0.0) if p == 0 else rng.uniform(-size, size, 2)
                x = np.round(np.clip(cx + ox + rr * np.cos(ang), 0, w), 2); y = np.round(np.clip(cy + oy + rr * np.sin(ang), 0, h), 2)
                polys.append(np.stack([x, y], 1).reshape(-1).tolist())
            anns.append({"id": aid, "image_id": i + 1, "category_id": int(rng.integers(1, 81)), "iscrowd": 0, "area": None,
                         "bbox": [float(max(0.0, cx - size)), float(max(0.0, cy - size)), float(2 * size), float(2 * size)], "segmentation": polys})
            aid += 1
    return {"images": images, "annotations": anns, "categories": [{"id": c} for c in range(1, 81)]}


def spread(ts):
    ts = sorted(ts)
    return ts[0] * 1e3, ts[len(ts) // 2] * 1e3, ts[-1] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--score-batches", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_encode_ab.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gt_encode_ab.py measures on the GPU: no device")               # never a CPU figure in its place
    CE = importlib.import_module("mask-rcnn-coreml_amd.coco_eval")
    ds = synthetic_annotations(args.images, args.seed)
    n_ann = len(ds["annotations"])
    n_poly = sum(len(a["segmentation"]) for a in ds["annotations"])
    n_vert = sum(len(p) // 2 for a in ds["annotations"] for p in a["segmentation"])
    lines = [f"git_head {git_head()}", f"device {torch.cuda.get_device_name(0)}",
             f"set: seed {args.seed}, {args.images} images of {len(SIZES)} sizes, {n_ann} annotations, {n_poly} polygons, {n_vert} vertices"]

    def leg_a():
        gt = CE.COCOGroundTruth(ds)
        t0 = time.perf_counter()
        out = [gt.counts(a) for anns in gt.by_image.values() for a in anns]
        return time.perf_counter() - t0, out

    def leg_b():
        gt = CE.COCOGroundTruth(ds)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = gt.to_device()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    # agreement first, bit for bit
    _, a = leg_a()
    _, b = leg_b()
    offs = b.run_offsets.cpu().numpy(); counts = b.counts.cpu().numpy().view(np.uint32)
    assert offs[-1] == sum(c.size for c in a) and np.array_equal(counts[:offs[-1]], np.concatenate(a)), "the legs disagree"
    assert np.array_equal(np.diff(offs), [c.size for c in a])
    runs = int(offs[-1])
    big = int((np.diff(offs) > CE.LDS_TOGGLES + 1).sum())
    lines.append(f"agreement: {n_ann} RLEs, {runs} runs ({runs * 4 / 1e6:.1f} MB), bit for bit; RLEs of more than {CE.LDS_TOGGLES + 1} runs: {big}")
    ta, tb = [], []
    for step in range(args.warmup + args.repeats):
        for leg, ts in ((leg_a, ta), (leg_b, tb)):
            t, _ = leg()
            if step >= args.warmup:
                ts.append(t)
    (a0, a1, a2), (b0, b1, b2) = spread(ta), spread(tb)
    lines.append(f"A host, COCOGroundTruth.counts() per annotation   ms min/median/max  {a0:.1f} / {a1:.1f} / {a2:.1f}   ({n_ann / a1 * 1e3:.0f} annotations/s)")
    lines.append(f"B device, COCOGroundTruth.to_device()             ms min/median/max  {b0:.1f} / {b1:.1f} / {b2:.1f}   ({n_ann / b1 * 1e3:.0f} annotations/s)")
    lines.append(f"A / B (medians) {a1 / b1:.2f}; warm-up rounds {args.warmup}, timed rounds {args.repeats}, legs alternating")
    if args.score:
        rng = np.random.default_rng(args.seed + 1)
        B, rows, H, W = 8, 100, 1024, 1024
        batches = []
        for s in range(args.score_batches):
            ids = [1 + s * B + b for b in range(B)]
            sizes = [(ds["images"][i - 1]["height"], ds["images"][i - 1]["width"]) for i in ids]
            det = np.zeros((B, rows, 6), np.float32)
            y1 = rng.random((B, rows)) * 0.5 + 0.2; x1 = rng.random((B, rows)) * 0.5 + 0.2
            det[..., 0], det[..., 1] = y1, x1
            det[..., 2] = np.minimum(0.8, y1 + 0.02 + rng.random((B, rows)) * 0.3); det[..., 3] = np.minimum(0.8, x1 + 0.02 + rng.random((B, rows)) * 0.3)
            det[..., 4] = rng.integers(1, 81, (B, rows)); det[..., 5] = 0.3 + 0.7 * rng.random((B, rows))
            yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
            cy = rng.uniform(8, 20, (B, rows, 1, 1)); cx = rng.uniform(8, 20, (B, rows, 1, 1)); sg = rng.uniform(5, 12, (B, rows, 1, 1))
            masks = np.exp(-(((yy - cy) / sg) ** 2 + ((xx - cx) / sg) ** 2)).astype(np.float32)
            batches.append(CE.device_detections(ids, torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, H, W, 0.5))
        img_ids = [i for b in batches for i in b.image_ids]
        gt = CE.COCOGroundTruth(ds)
        for anns in gt.by_image.values():                                          # the host encodings exist already: A pays only concatenation and upload
            for an in anns:
                gt.counts(an)
        resident = gt.to_device()

        def timed(**kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = CE.score_batch(gt, batches, "segm", img_ids=img_ids, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        _, p = timed()
        _, q = timed(device_gt=resident)
        assert all(np.array_equal(p[k], q[k]) for k in ("precision", "recall", "stats")), "the scores disagree"
        sa, sb = [], []
        for step in range(args.warmup + args.repeats):
            for kw, ts in (({}, sa), ({"device_gt": resident}, sb)):
                t, _ = timed(**kw)
                if step >= args.warmup:
                    ts.append(t)
        (a0, a1, a2), (b0, b1, b2) = spread(sa), spread(sb)
        lines.append(f"score_batch segm, {len(batches)} batches of {B} x {rows} rows, ground truth of {len(img_ids)} images; the same twelve numbers")
        lines.append(f"A ground truth uploaded per batch (host encodings cached)   ms min/median/max  {a0:.1f} / {a1:.1f} / {a2:.1f}")
        lines.append(f"B resident ground truth                                     ms min/median/max  {b0:.1f} / {b1:.1f} / {b2:.1f}")
        lines.append(f"A / B (medians) {a1 / b1:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
