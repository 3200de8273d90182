"""The set algebra of run-length masks: what mrcnn_rle_combine costs on device-resident runs against the route a host has without it,
in one process on the GPU.

  rle_combine_ab.py [--steps 20] [--warmup 3] [--host-steps 1] [--out profiles/rle_combine_ab.json]

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  work    disjoint   detection.rle_disjoint: row i minus every drawn row before it — groups of up to `slots` members, one call
          union      detection.rle_union, pairwise: every row united with the row after it in the set (the last with the first)
  legs    device   on the device-resident (counts, run_offsets) pair: the result stays on the device.  rle_disjoint reads the rows
                   back to decide which are drawn and builds the group tables on the host: that is part of the call and is timed
          host     the route a host has without the entry: the runs copied down, the sequential definition there (a plane per member,
                   folded pixel by pixel), the result copied back to the device.  The definition is written to be read, not to be
                   fast — it decodes a plane for every member of every group — so the ratio says what the entry saves a host that has
                   nothing else, not how it compares with an optimised host merge.  The first call is timed (no warm-up), and
                   --host-steps - 1 more only if that first call took under 20 s

Before anything is timed every device result is compared with the host definition's, array by array.  Every figure is the median of
the timed calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end synchronised.
There is no pass bar; the result says which leg won and is written down as it is."""
import argparse, importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_components_ab import flat, timed  # noqa: E402
from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

WORK = ("disjoint", "union")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--scenes", default="tiled,batch")
    ap.add_argument("--git", default=None, help="the commit the record belongs to, where the tree that runs has no history of its own")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_combine_ab.json"))
    args = ap.parse_args()
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")

    scenes = {}
    if "tiled" in args.scenes:
        tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
        odet, omask, _n_objects = objects_scene(tiles, 100)
        out = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
        scenes["tiled"] = (out[0], out[3], [(H_IMG, W_IMG)])
    if "batch" in args.scenes:
        bdet, bmask, bsizes = batch_scene()
        out = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
        scenes["batch"] = (out[0], out[1], bsizes)
    rec = {"git": args.git or git_head(), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "scenes": {}}
    ok = True
    for name, (det_src, rles, sizes) in scenes.items():
        det_src = np.asarray(det_src, np.float32)
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        n = len(offs) - 1
        nxt = np.roll(np.arange(n), -1)                          # the set rolled by one: its RLE k is RLE k + 1
        other_c = np.concatenate([counts[offs[k]:offs[k + 1]] for k in nxt]) if n else counts
        other_o = np.concatenate(([0], np.cumsum([offs[k + 1] - offs[k] for k in nxt]))).astype(np.int64)
        slots = len(rles[0])
        if len({tuple(s) for s in sizes}) > 1:                   # (rolling crosses images: only sets of one size can be united pairwise this way)
            raise SystemExit("the scenes' images are expected to have one size")
        cuda = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        pair, other, det_g = (cuda(counts), cuda(offs)), (cuda(other_c), cuda(other_o)), cuda(det_src)
        torch.cuda.synchronize()
        device = {"disjoint": lambda: D.rle_disjoint(det_g, pair, sizes), "union": lambda: D.rle_union(pair, sizes, other=other)}

        def down(p):
            return p[0].cpu().numpy().view(np.uint32), p[1].cpu().numpy()

        def up(result):
            return [cuda(a) for a in flat(result)]
        host = {"disjoint": lambda: up(D.rle_disjoint_host(det_g.cpu().numpy(), down(pair), sizes)),
                "union": lambda: up(D.rle_union_host(down(pair), sizes, other=down(other)))}
        ms = {"device": {}, "host": {}}
        same, host_calls = {}, {}
        got = {w: device[w]() for w in WORK}
        for w in WORK:
            t0 = time.perf_counter()
            want = host[w]()
            first = time.perf_counter() - t0
            print(f"{name}: the host route of {w} took {first:.1f} s", file=sys.stderr, flush=True)
            same[w] = all(np.array_equal(g, h.cpu().numpy().view(g.dtype)) for g, h in zip(flat(got[w]), want)) and len(flat(got[w])) == len(want)
            ok = ok and same[w]
            more = timed(host[w], 0, args.host_steps - 1) if args.host_steps > 1 and first < 20.0 else []
            ms["host"][w] = stats([first] + more)
            host_calls[w] = 1 + len(more)
        for w in WORK:
            ms["device"][w] = stats(timed(device[w], args.warmup, args.steps))
        drawn = D.drawn_rows(det_src, sizes, 0.0)
        members = int(sum(1 + int(drawn[b, :i].sum()) if drawn[b, i] else 2 for b in range(len(sizes)) for i in range(slots)))
        dis = flat(got["disjoint"])
        rec["scenes"][name] = {"images": len(sizes), "size": list(sizes[0]), "slots": slots, "runs_in": int(counts.size), "drawn_rows": int(drawn.sum()),
                               "disjoint_members": members, "disjoint_runs_out": int(dis[0].size), "pixels_before": sum(int(counts[offs[k]:offs[k + 1]][1::2].sum()) for k in range(n)), "pixels_disjoint": int(dis[2].astype(np.int64).sum()),
                               "union_runs_out": int(flat(got["union"])[0].size), "plane_bytes_a_host_decodes": {"disjoint": int(members * sizes[0][0] * sizes[0][1]),
                                                                                                                  "union": int(2 * n * sizes[0][0] * sizes[0][1])},
                               "arrays_equal": same, "host_calls": host_calls, "ms": ms,
                               "host_over_device": {w: ms["host"][w]["median"] / ms["device"][w]["median"] for w in WORK}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
