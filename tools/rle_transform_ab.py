"""Moving run-length masks to another pixel grid: what mrcnn_rle_transform costs on device-resident runs against the route a host has
without it, in one process on the GPU.

  rle_transform_ab.py [--steps 20] [--warmup 3] [--host-steps 1] [--out profiles/rle_transform_ab.json]

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  work    crop     detection.rle_crop to the central half of every image (a quarter of its pixels)
          flip     detection.rle_flip, horizontal
          rot90    detection.rle_rot90, k = 1: transposed records, the kernel's point-query form
          resize   detection.rle_resize to a quarter of each side, the pixel-centre rule
  legs    device   on the device-resident (counts, run_offsets) pair: the result stays on the device
          host     the route a host has without the entry: the runs copied down, the sequential definition there (a plane per RLE,
                   the forward rule pixel by pixel), the result copied back to the device.  The definition is written to be read, not
                   to be fast, so the ratio says what the entry saves a host that has nothing else, not how it compares with an
                   optimised host routine.  One call is timed (no warm-up), and --host-steps - 1 more only if the first took under 20 s

Before anything is timed every device result is compared with the host definition's, array by array.  Every device figure is the
median of the timed calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end
synchronised.  There is no pass bar; the result says which leg won and is written down as it is."""
import argparse, importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_components_ab import flat, timed  # noqa: E402
from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

WORK = ("crop", "flip", "rot90", "resize")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--scenes", default="tiled,batch")
    ap.add_argument("--git", default=None, help="the commit the record belongs to, where the tree that runs has no history of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_transform_ab.json"))
    args = ap.parse_args()
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")

    scenes = {}
    if "tiled" in args.scenes:
        tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
        odet, omask, _n_objects = objects_scene(tiles, 100)
        out = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
        scenes["tiled"] = (out[3], [(H_IMG, W_IMG)])
    if "batch" in args.scenes:
        bdet, bmask, bsizes = batch_scene()
        out = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
        scenes["batch"] = (out[1], bsizes)
    rec = {"git": args.git or git_head(), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "scenes": {}}
    ok = True
    for name, (rles, sizes) in scenes.items():
        sizes = [(int(h), int(w)) for h, w in sizes]
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        n = len(offs) - 1
        cuda = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        pair = (cuda(counts), cuda(offs))
        torch.cuda.synchronize()
        windows = [(w // 4, h // 4, w // 2, h // 2) for h, w in sizes]
        quarter = [(h // 4, w // 4) for h, w in sizes]

        def down(p):
            return p[0].cpu().numpy().view(np.uint32), p[1].cpu().numpy()

        def up(result):
            return [cuda(a) for a in flat(result[:3])]
        device = {"crop": lambda: D.rle_crop(pair, sizes, windows), "flip": lambda: D.rle_flip(pair, sizes, horizontal=True),
                  "rot90": lambda: D.rle_rot90(pair, sizes, 1), "resize": lambda: D.rle_resize(pair, sizes, quarter)}
        host = {"crop": lambda: up(D.rle_crop_host(down(pair), sizes, windows)), "flip": lambda: up(D.rle_flip_host(down(pair), sizes, horizontal=True)),
                "rot90": lambda: up(D.rle_rot90_host(down(pair), sizes, 1)), "resize": lambda: up(D.rle_resize_host(down(pair), sizes, quarter))}
        ms = {"device": {}, "host": {}}
        same, host_calls, runs_out, pixels_out = {}, {}, {}, {}
        got = {w: device[w]() for w in WORK}
        for w in WORK:
            t0 = time.perf_counter()
            want = host[w]()
            first = time.perf_counter() - t0
            print(f"{name}: the host route of {w} took {first:.1f} s", file=sys.stderr, flush=True)
            mine = flat(got[w][:3])
            same[w] = len(mine) == len(want) and all(np.array_equal(g, h.cpu().numpy().view(g.dtype)) for g, h in zip(mine, want))
            ok = ok and same[w]
            more = timed(host[w], 0, args.host_steps - 1) if args.host_steps > 1 and first < 20.0 else []
            ms["host"][w] = stats([first] + more)
            host_calls[w] = 1 + len(more)
            runs_out[w] = int(mine[0].size)
            pixels_out[w] = int(mine[2].astype(np.int64).sum())
        for w in WORK:
            ms["device"][w] = stats(timed(device[w], args.warmup, args.steps))
        rec["scenes"][name] = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "rles": n, "runs_in": int(counts.size),
                               "pixels_in": sum(int(counts[offs[k]:offs[k + 1]][1::2].sum()) for k in range(n)), "runs_out": runs_out, "pixels_out": pixels_out,
                               "plane_bytes_a_host_decodes": int(sum(h * w for h, w in sizes) * len(rles[0])),
                               "arrays_equal": same, "host_calls": host_calls, "ms": ms,
                               "host_over_device": {w: ms["host"][w]["median"] / ms["device"][w]["median"] for w in WORK}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
