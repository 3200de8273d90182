"""Tiled prediction: what the device paths cost against what a host had before, on one 4096x3072 image at the bench model
(ResNet-101, 1024x1024, 81 classes, synthetic weights), in one process on the GPU.

  tiled_ab.py [--steps 5] [--warmup 1] [--mode f16] [--batch 4] [--overlap 128] [--out profiles/tiled_ab.json]

  predict   A  the parent commit's only way: every window cropped on the CPU into a contiguous buffer (np.ascontiguousarray), the
               crops through predict_images max_batch at a time — the overlaps cross PCIe once per window
            B  predict_tiles: the image crosses once, the pre-processing reads the windows through the image's row pitch
  merge     A  mrcnn_merge_tiles_host (the sequential definition) on the records
            B  mrcnn_merge_tiles on the same host records (staging copies included)

  unite     A  mrcnn_unite_tiles_host (the sequential definition) on the same records
            B  mrcnn_unite_tiles on the same host records (staging copies included)
  unite_objects  the same pair on a second scene: synthetic objects larger than the overlap, one row in every window that sees a part
               of them, cut at the window's edge (as tests/tiles_cases.py builds its scenes) — the synthetic model's rows rarely link

Before anything is timed B's results are compared with A's bit for bit.  A and B alternate inside every step; every figure is the
median of --steps calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end
synchronised.  No ratio was promised for either pair; the result says which leg won."""
import argparse, importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")
H_IMG, W_IMG, MODEL = 3072, 4096, 1024


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def stats(ts):
    ts = sorted(ts)
    return {"min": ts[0] * 1e3, "median": ts[len(ts) // 2] * 1e3, "max": ts[-1] * 1e3}


def objects_scene(tiles, rows, S=28, seed=9):
    """Objects of 300..1500 pixels a side on the image: every window that sees at least 2 pixels of one gets a row with the part it
    sees (tiles of the model's size: the letterbox is the identity and the box comes out exactly).  Masks: full, or smooth noise."""
    rng = np.random.default_rng(seed)
    T = tiles.shape[0]
    det, masks, fill = np.zeros((T, rows, 6), np.float32), np.zeros((T, rows, S, S), np.float32), [0] * T
    n_objects = 0
    for j in range(60):
        oh, ow = (int(v) for v in rng.integers(300, 1500, 2))
        y1, x1 = int(rng.integers(0, H_IMG - oh)), int(rng.integers(0, W_IMG - ow))
        y2, x2, cls, score = y1 + oh, x1 + ow, int(rng.integers(1, 6)), 0.5 + 0.4 * float(rng.random())
        mask = np.full((S, S), 0.9, np.float32) if j % 3 else np.kron(rng.random((7, 7)).astype(np.float32), np.ones((4, 4), np.float32)) * 0.6 + 0.2
        n_objects += 1
        for t, (_, ty, tx, th, tw) in enumerate(tiles.tolist()):
            cy1, cx1, cy2, cx2 = max(y1, ty), max(x1, tx), min(y2, ty + th), min(x2, tx + tw)
            if fill[t] >= rows or cy2 - cy1 < 2 or cx2 - cx1 < 2:
                continue
            det[t, fill[t]] = [(cy1 - ty) / (MODEL - 1), (cx1 - tx) / (MODEL - 1), (cy2 - ty - 1) / (MODEL - 1), (cx2 - tx - 1) / (MODEL - 1), cls,
                               score - 0.001 * float(rng.integers(0, 3))]
            masks[t, fill[t]] = mask
            fill[t] += 1
    return det, masks, n_objects


def count_links(D, det, mask, tiles, metric, thr, group):
    """The links of the rule, counted on the host from the candidates' own run lists (a no-link run returns them): only candidates of
    one component can be linked, so only those pairs are measured."""
    T, rows = det.shape[:2]
    alone = D.unite_tiles_host(det, mask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 1.5, T * rows)
    ends = {int(k): np.cumsum(alone[3][0][j]["counts"].astype(np.int64)) for j, k in enumerate(alone[1][0]) if k >= 0}

    def inside(r, n):                                            # positions p < n (p = x*h + y) inside rows [y0, y1), columns [x0, x1)
        x, y = n // H_IMG, n % H_IMG
        return np.clip(x - r[1], 0, r[3] - r[1]) * (r[2] - r[0]) + np.where((x >= r[1]) & (x < r[3]), np.clip(y - r[0], 0, r[2] - r[0]), 0)
    g = group.reshape(-1)
    links = 0
    for c in np.unique(g[g >= 0]):
        mem = np.flatnonzero(g == c).tolist()
        for i, q in enumerate(mem):
            for k in mem[i + 1:]:
                tq, tk = tiles[q // rows], tiles[k // rows]
                r = (max(tq[1], tk[1]), max(tq[2], tk[2]), min(tq[1] + tq[3], tk[1] + tk[3]), min(tq[2] + tq[4], tk[2] + tk[4]))
                if q // rows == k // rows or det.reshape(-1, 6)[q, 4] != det.reshape(-1, 6)[k, 4] or r[2] <= r[0] or r[3] <= r[1]:
                    continue
                cut = np.union1d(ends[q], ends[k])                # segment ends; a segment lies in one run of either list
                lo = np.concatenate(([0], cut[:-1]))
                in_q, in_k = np.searchsorted(ends[q], lo, "right") & 1, np.searchsorted(ends[k], lo, "right") & 1
                f = inside(r, cut) - inside(r, lo)
                inter, aq, ak = int(((cut - lo) * (in_q & in_k)).sum()), int((f * in_q).sum()), int((f * in_k).sum())
                den = aq + ak - inter if metric == "iou" else min(aq, ak)
                links += den > 0 and inter / den >= thr
    return int(links)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", default="f16")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_ab.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    cfg = pkg.ModelConfig(architecture="resnet101", input_image_shape=(MODEL, MODEL, 3), num_classes=81, pre_nms_max_proposals=6000)
    d = tempfile.mkdtemp(prefix="tiled_ab_")
    weights.save_synthetic_models(d, cfg, seed=0, forced_load=True)
    m = models.load_maskrcnn(d, max_batch=args.batch, compute_dtype=args.mode)
    rng = np.random.default_rng(5)
    # smooth structure under noise: a synthetic model finds more on it than on white noise
    base = rng.integers(0, 256, (H_IMG // 64, W_IMG // 64, 3)).astype(np.uint8)
    image = np.kron(base, np.ones((64, 64, 1), np.uint8)) ^ rng.integers(0, 32, (H_IMG, W_IMG, 3), dtype=np.uint8)
    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (args.overlap, args.overlap))
    T = int(tiles.shape[0])

    def leg_crops():
        crops = [np.ascontiguousarray(image[y:y + h, x:x + w]) for _, y, x, h, w in tiles.tolist()]
        out = [m.predict_images(crops[i:i + args.batch]) for i in range(0, T, args.batch)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    def leg_tiles():
        return m.predict_tiles([image], tiles)
    det_a, mask_a = leg_crops()
    det, mask = leg_tiles()
    same_predict = bool(np.array_equal(det_a, det) and np.array_equal(mask_a, mask))
    merge = lambda f: f(det, mask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "ios", 0.5, None)
    host, dev = merge(D.merge_tiles_host), merge(D.merge_tiles)
    same_merge = bool(all(np.array_equal(a, b) for a, b in zip(host[:3] + host[4:], dev[:3] + dev[4:])) and
                      all(np.array_equal(a["counts"], b["counts"]) for a, b in zip(host[3][0], dev[3][0])))
    same = lambda a, b: bool(all(np.array_equal(x, y) for x, y in zip(a[:3] + a[4:], b[:3] + b[4:])) and
                             all(np.array_equal(x["counts"], y["counts"]) for x, y in zip(a[3][0], b[3][0])))
    unite = lambda f: f(det, mask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    uhost, udev = unite(D.unite_tiles_host), unite(D.unite_tiles)
    odet, omask, n_objects = objects_scene(tiles, m.max_detections, int(mask.shape[2]))
    ounite = lambda f: f(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    ohost, odev = ounite(D.unite_tiles_host), ounite(D.unite_tiles)
    same_unite, same_objects = same(uhost, udev), same(ohost, odev)
    times = {k: [] for k in ("predict_crops", "predict_tiles", "merge_host", "merge_device", "unite_host", "unite_device", "unite_objects_host",
                             "unite_objects_device")}
    for step in range(args.warmup + args.steps):
        for name, leg in (("predict_crops", leg_crops), ("predict_tiles", leg_tiles), ("merge_host", lambda: merge(D.merge_tiles_host)),
                          ("merge_device", lambda: merge(D.merge_tiles)), ("unite_host", lambda: unite(D.unite_tiles_host)),
                          ("unite_device", lambda: unite(D.unite_tiles)), ("unite_objects_host", lambda: ounite(D.unite_tiles_host)),
                          ("unite_objects_device", lambda: ounite(D.unite_tiles))):
            t0 = time.perf_counter()
            leg()
            if step >= args.warmup:
                times[name].append(time.perf_counter() - t0)
    rec = {"git": git_head(), "image": [H_IMG, W_IMG], "model": MODEL, "mode": m.compute_dtype, "max_batch": args.batch, "overlap": args.overlap,
           "tiles": T, "candidates": T * m.max_detections, "detections": int((det[..., 5] > 0).sum()), "kept": int(dev[2][0]),
           "predict_bits_equal": same_predict, "merge_bits_equal": same_merge, "steps": args.steps, "warmup": args.warmup,
           "unite_bits_equal": same_unite, "unite_objects_bits_equal": same_objects,
           "unite": {"metric": "iou", "link_threshold": 0.5, "components": int(udev[2][0]), "united": int((udev[6] > 1).sum()),
                     "links": count_links(D, det, mask, tiles, "iou", 0.5, udev[7])},
           "unite_objects": {"objects": n_objects, "candidates": int((odet[..., 5] > 0).sum()), "components": int(odev[2][0]),
                             "united": int((odev[6] > 1).sum()), "most_parts": int(odev[6].max()), "links": count_links(D, odet, omask, tiles, "iou", 0.5, odev[7])},
           "ms": {k: stats(v) for k, v in times.items()}}
    rec["predict_tiles_over_crops"] = rec["ms"]["predict_crops"]["median"] / rec["ms"]["predict_tiles"]["median"]
    rec["merge_device_over_host"] = rec["ms"]["merge_host"]["median"] / rec["ms"]["merge_device"]["median"]
    rec["unite_device_over_host"] = rec["ms"]["unite_host"]["median"] / rec["ms"]["unite_device"]["median"]
    rec["unite_objects_device_over_host"] = rec["ms"]["unite_objects_host"]["median"] / rec["ms"]["unite_objects_device"]["median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if same_predict and same_merge and same_unite and same_objects else 1


if __name__ == "__main__":
    sys.exit(main())
