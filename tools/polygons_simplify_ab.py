"""Simplified polygons out: what trace + mrcnn_polygons_simplify costs on the device against the route a host has without it, in one
process on the GPU.

  polygons_simplify_ab.py [--steps 20] [--warmup 3] [--out profiles/polygons_simplify_ab.json]

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  legs    device   detection.rle_to_polygons(tolerance=t) on the device-resident (counts, run_offsets) pair: traced and simplified where
                   the runs lie, the simplified rings left on the device.  simplify alone is timed beside it (detection.simplify_polygons
                   on the traced tensors)
          host     the route a host has today: the rings traced on the device, all vertices copied to the host, the sequential
                   definition there (mrcnn_polygons_simplify_host), the result kept on the host
  tolerances 0.5, 1 and 2 px

Before anything is timed the device result is compared with the host definition's, array by array.  The legs alternate inside every
step; every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it, taken with a host clock
around calls that end synchronised.  `rounds` is the largest number of rounds one ring's workgroup loops: one more than the deepest
level of the recursion, counted on the host from the kept sets.  No time was promised for either route; the result says which leg
won, and if the device loses at the small scene that is written down as it is: the point is that the rings need not leave the device."""
import argparse, importlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

KEYS = ("ring_offsets", "areas2", "xy", "src_index")
TOLERANCES = (0.5, 1.0, 2.0)


def rounds_of(ring_offsets, xy, src_index, out_offsets):
    """The rounds the deepest ring needs: a chain's level is one more than the level of the chain it was cut from, and a ring loops once
    per level and once more to see that nothing is left.  Rebuilt from the kept sets: in a chain a .. b the kept vertex of largest
    distance from the chord (the first of equals) is the one the chain was cut at."""
    most = 0
    for r in range(len(ring_offsets) - 1):
        v0, m = int(ring_offsets[r]), int(ring_offsets[r + 1] - ring_offsets[r])
        kept = (src_index[int(out_offsets[r]):int(out_offsets[r + 1])] - v0).astype(np.int64)
        if m <= 2 or len(kept) < 2:
            continue
        p = np.concatenate((xy[v0:v0 + m], xy[v0:v0 + 1])).astype(np.int64)
        idx = np.concatenate((kept, [m]))                        # vertex m is vertex 0 again
        f = int(np.argmax(((p[kept] - p[0]) ** 2).sum(1)))       # the second anchor is kept, and no kept vertex lies farther from the first
        stack = [(0, f, 1), (f, len(kept), 1)]                   # positions in idx
        deepest = 0
        while stack:
            i, j, level = stack.pop()
            a, b = int(idx[i]), int(idx[j])
            if b - a < 2:
                continue
            deepest = max(deepest, level)
            if j - i < 2:
                continue
            q = idx[i + 1:j]
            c = np.abs((p[b, 0] - p[a, 0]) * (p[q, 1] - p[a, 1]) - (p[b, 1] - p[a, 1]) * (p[q, 0] - p[a, 0]))
            k = i + 1 + int(np.argmax(c))
            stack += [(i, k, level + 1), (k, j, level + 1)]
        most = max(most, deepest + 1)
    return most


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_simplify_ab.json"))
    args = ap.parse_args()
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    limit = importlib.import_module("mask-rcnn-coreml_amd._lib").SIMPLIFY_LDS_VERTICES

    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
    odet, omask, n_objects = objects_scene(tiles, 100)
    united = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    bdet, bmask, bsizes = batch_scene()
    encoded = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
    scenes = {"tiled": (united[3], [(H_IMG, W_IMG)]), "batch": (encoded[1], bsizes)}
    rec = {"git": git_head(), "steps": args.steps, "warmup": args.warmup, "scenes": {}}
    ok = True
    for name, (rles, sizes) in scenes.items():
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())
        traced = D.rle_to_polygons(pair, sizes, flat=True)
        torch.cuda.synchronize()
        sizes_in = np.diff(traced["ring_offsets"].cpu().numpy())
        scene = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "rings": traced["n_rings"], "vertices": traced["n_vertices"],
                 "most_vertices": int(sizes_in.max()), "rings_above_the_lds_limit": int((sizes_in > limit).sum()), "tolerances": {}}
        for tol in TOLERANCES:
            def device():
                out = D.rle_to_polygons(pair, sizes, flat=True, tolerance=tol)
                torch.cuda.synchronize()
                return out

            def simplify():
                out = D.simplify_polygons(traced, tol)
                torch.cuda.synchronize()
                return out

            def host():
                t = D.rle_to_polygons(pair, sizes, flat=True)
                return D.simplify_polygons_host({"ring_offsets": t["ring_offsets"].cpu().numpy(), "xy": t["xy"].cpu().numpy()}, tol)
            got, want = device(), host()
            same = bool(all(np.array_equal(got[k].cpu().numpy().reshape(-1), want[k].reshape(-1)) for k in KEYS))
            ok = ok and same
            legs = (("device", device), ("simplify_alone", simplify), ("host", host))
            times = {k: [] for k, _ in legs}
            for step in range(args.warmup + args.steps):
                for k, leg in legs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    leg()
                    if step >= args.warmup:
                        times[k].append(time.perf_counter() - t0)
            ms = {k: stats(v) for k, v in times.items()}
            scene["tolerances"][str(tol)] = {"vertices_after": want["n_vertices"], "arrays_equal": same, "ms": ms,
                                             "rounds": rounds_of(traced["ring_offsets"].cpu().numpy(), traced["xy"].cpu().numpy(), want["src_index"],
                                                                 want["ring_offsets"]),
                                             "host_over_device": ms["host"]["median"] / ms["device"]["median"]}
        rec["scenes"][name] = scene
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
