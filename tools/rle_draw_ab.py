"""Drawing run-length masks: what the device entries cost against the route a user had before, in one process on the GPU.

  rle_draw_ab.py [--steps 20] [--warmup 3] [--out profiles/rle_draw_ab.json]

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots, 92 components
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source
  legs    map_device / render_device   mrcnn_instance_map_rle / mrcnn_render_detections_rle on device-resident rows, runs and images
                                       (the whole entry: prefix pass, records, the check's one word read back, the draw)
          map_host / render_host       the only route before: the runs to the host, the sequential _host definition, the result copied
                                       back to the device (where jpeg.encode_batch / png.encode_batch take it)

Before anything is timed the device results are compared with the host definition's byte for byte.  The legs alternate inside every
step; every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it, taken with a host clock
around calls that end synchronised.  `map_bytes_per_s` is the map's algorithmic 2*h*w bytes over the ENTRY's median time — the kernel's
own time comes from a `rocprofv3 --kernel-trace --stats` run of this tool (kernels k_rle_prefix, k_rle_draw_prepare, k_rle_draw).  No
ratio was promised; the result says which leg won."""
import argparse, importlib, json, os, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402


def batch_scene(B=8, h=480, w=640, rows=100, S=28, seed=13):
    """Rows in the letterboxed frame of a MODEL x MODEL model with smooth blob masks, scores descending."""
    E = importlib.import_module("mask-rcnn-coreml_amd.evaluate")
    rng = np.random.default_rng(seed)
    nh, nw, py, px = E.letterbox_geometry(h, w, MODEL, MODEL)
    det, masks = np.zeros((B, rows, 6), np.float32), np.zeros((B, rows, S, S), np.float32)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    for b in range(B):
        y1, x1 = rng.random(rows) * 0.7, rng.random(rows) * 0.7
        y2, x2 = np.minimum(1.0, y1 + 0.05 + rng.random(rows) * 0.4), np.minimum(1.0, x1 + 0.05 + rng.random(rows) * 0.4)
        det[b, :, 0], det[b, :, 2] = (py + y1 * nh) / (MODEL - 1), (py + y2 * nh) / (MODEL - 1)
        det[b, :, 1], det[b, :, 3] = (px + x1 * nw) / (MODEL - 1), (px + x2 * nw) / (MODEL - 1)
        det[b, :, 4], det[b, :, 5] = rng.integers(1, 80, rows), np.linspace(0.99, 0.35, rows)
        for i in range(rows):
            cy, cx, sy, sx = *rng.uniform(8, 20, 2), *rng.uniform(4, 9, 2)
            masks[b, i] = np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
    return det, masks, [(h, w)] * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_draw_ab.json"))
    args = ap.parse_args()
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    rng = np.random.default_rng(5)

    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
    odet, omask, n_objects = objects_scene(tiles, 100)
    united = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    bdet, bmask, bsizes = batch_scene()
    encoded = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
    scenes = {"tiled": (united[0], united[3], [(H_IMG, W_IMG)], {"objects": n_objects, "components": int(united[2][0])}),
              "batch": (encoded[0], encoded[1], bsizes, {})}
    rec = {"git": git_head(), "steps": args.steps, "warmup": args.warmup, "scenes": {}}
    ok = True
    for name, (det_src, rles, sizes, extra) in scenes.items():
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        det_g, images_g = torch.from_numpy(det_src).cuda(), [torch.from_numpy(im).cuda() for im in images]
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())

        def map_device():
            return D.instance_map_rle(det_g, pair, sizes, 0.0)

        def render_device():
            return D.render_detections_rle(images_g, det_g, pair, 0.7, 128, 3)

        def host_set():                                                      # the runs and the rows come to the host
            return det_g.cpu().numpy(), (pair[0].cpu().numpy().view(np.uint32), pair[1].cpu().numpy())

        def map_host():
            d, p = host_set()
            maps, vis = D.instance_map_rle_host(d, p, sizes, 0.0)
            out = [torch.from_numpy(m).cuda() for m in maps], torch.from_numpy(vis.view(np.int32)).cuda()
            torch.cuda.synchronize()
            return out

        def render_host():
            d, p = host_set()
            out = [torch.from_numpy(r).cuda() for r in D.render_detections_rle_host(images, d, p, 0.7, 128, 3)]
            torch.cuda.synchronize()
            return out
        (m_d, v_d), (m_h, v_h), r_d, r_h = map_device(), map_host(), render_device(), render_host()
        same_map = bool(all(torch.equal(a, b) for a, b in zip(m_d, m_h)) and torch.equal(v_d, v_h))
        same_render = bool(all(torch.equal(a, b) for a, b in zip(r_d, r_h)))
        ok = ok and same_map and same_render
        legs = (("map_device", map_device), ("map_host", map_host), ("render_device", render_device), ("render_host", render_host))
        times = {k: [] for k, _ in legs}
        for step in range(args.warmup + args.steps):
            for k, leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                if step >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
        pixels = sum(h * w for h, w in sizes)
        ms = {k: stats(v) for k, v in times.items()}
        rec["scenes"][name] = dict(extra, images=len(sizes), size=list(sizes[0]), slots=int(det_src.shape[1]), runs=int(counts.size),
                                   drawn_rows_map=int((det_src[..., 5] > 0).sum()), drawn_rows_render=int((det_src[..., 5] > 0.7).sum()),
                                   owned_pixels=int(v_d.sum().item()), pixels=pixels, map_bytes_equal=same_map, render_bytes_equal=same_render, ms=ms,
                                   map_device_over_host=ms["map_host"]["median"] / ms["map_device"]["median"],
                                   render_device_over_host=ms["render_host"]["median"] / ms["render_device"]["median"],
                                   map_algorithmic_bytes=2 * pixels, map_bytes_per_s=2 * pixels / (ms["map_device"]["median"] * 1e-3),
                                   render_algorithmic_bytes=6 * pixels, render_bytes_per_s=6 * pixels / (ms["render_device"]["median"] * 1e-3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
