"""Measuring run-length masks: what mrcnn_rle_measure and mrcnn_rle_convex_hull cost on device-resident runs against the route a host
has without them, in one process on the GPU.

  rle_shape_ab.py [--steps 20] [--warmup 3] [--host-steps 3] [--out profiles/rle_shape_ab.json]

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  work    measure  detection.rle_measure: the six moments and the perimeter of every RLE
          hull     detection.rle_convex_hull(flat=True): the hulls, their areas and the oriented boxes
          props    detection.rle_region_props: both, the small tables read back, the doubles made on the host
  legs    device   on the device-resident (counts, run_offsets) pair: the tables of measure and hull stay on the device
          host     the route a host has without the entries: the runs copied down, the sequential definitions there, the tables copied
                   back to the device (measure, hull).  The definitions are written to be read — the moments are summed pixel by
                   pixel — but they never build a plane either, so the ratio is against a host that already works on the runs, not
                   against regionprops on decoded planes

Before anything is timed every device table is compared with the host definition's, array by array.  Every figure is the median of
the timed calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end synchronised.
There is no pass bar; the result says which leg won and is written down as it is."""
import argparse, importlib, json, os, sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_components_ab import flat, timed  # noqa: E402
from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

WORK = ("measure", "hull", "props")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--scenes", default="tiled,batch")
    ap.add_argument("--git", default=None, help="the commit the record belongs to, where the tree that runs has no history of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_shape_ab.json"))
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
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        n = len(offs) - 1
        cuda = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        pair = (cuda(counts), cuda(offs))
        torch.cuda.synchronize()
        down = lambda: (pair[0].cpu().numpy().view(np.uint32), pair[1].cpu().numpy())
        up = lambda result: [cuda(np.ascontiguousarray(a)) for a in flat(result if isinstance(result, tuple) else (result,))]
        device = {"measure": lambda: D.rle_measure(pair, sizes), "hull": lambda: D.rle_convex_hull(pair, sizes, flat=True),
                  "props": lambda: D.rle_region_props(pair, sizes)}
        host = {"measure": lambda: up(D.rle_measure_host(down(), sizes)), "hull": lambda: up(D.rle_convex_hull_host(down(), sizes, flat=True)),
                "props": lambda: D.rle_region_props_host(down(), sizes)}
        same = {}
        for w in WORK:
            got, want = device[w](), host[w]()
            if w == "props":
                same[w] = sorted(got) == sorted(want) and all(got[k].tobytes() == want[k].tobytes() for k in got)
            else:
                got = flat(got if isinstance(got, tuple) else (got,))
                same[w] = len(got) == len(want) and all(np.array_equal(g, h.cpu().numpy().view(g.dtype)) for g, h in zip(got, want))
            ok = ok and same[w]
        ms = {"device": {w: stats(timed(device[w], args.warmup, args.steps)) for w in WORK},
              "host": {w: stats(timed(host[w], 1, args.host_steps)) for w in WORK}}
        m = D.rle_measure_host(down(), sizes)
        hull = D.rle_convex_hull_host(down(), sizes, flat=True)
        rec["scenes"][name] = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "rles": n, "runs_in": int(counts.size),
                               "masks_with_pixels": int((m[:, 0] > 0).sum()), "pixels": int(m[:, 0].sum()), "hull_vertices": int(hull[0][-1]),
                               "most_hull_vertices": int(np.diff(hull[0]).max()) if n else 0,
                               "plane_bytes_a_regionprops_host_decodes": int(sum(int(h) * int(w) for h, w in sizes) * len(rles[0])),
                               "arrays_equal": same, "ms": ms, "host_over_device": {w: ms["host"][w]["median"] / ms["device"][w]["median"] for w in WORK}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
