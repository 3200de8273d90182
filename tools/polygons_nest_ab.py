"""Nested polygons out: what trace + mrcnn_polygons_nest costs on the device against the route a host has without it, in one process on
the GPU.

  polygons_nest_ab.py [--steps 20] [--warmup 3] [--only nest] [--out profiles/polygons_nest_ab.json]
  polygons_nest_ab.py --share profiles/polygons_nest_ab_only.json <kernel_stats.csv>

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  legs    device   detection.rle_to_polygons(nest=True) on the device-resident (counts, run_offsets) pair: traced and nested where the
                   runs lie, rings and nesting left on the device.  nest alone is timed beside it (detection.nest_polygons on the traced
                   tensors)
          host     the route a host has without the entry: the rings traced on the device, all vertices copied to the host, the
                   sequential definition there (mrcnn_polygons_nest_host), the result kept on the host

Before anything is timed the device result is compared with the host definition's, array by array.  The legs alternate inside every
step; every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it, taken with a host clock
around calls that end synchronised.  The kernels' share of a nest call comes from a second run: `rocprofv3 --kernel-trace --stats
--output-format csv` around `polygons_nest_ab.py --only nest`, whose kernel_stats.csv `--share` divides by that run's calls and medians
(kernels k_nest_*).
No time was promised for either route; the result says which leg won, and if the device loses that is written down as it is: the
point is that the rings need not leave the device."""
import argparse, csv, importlib, json, os, re, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

KEYS = ("parent", "depth", "rle_polys", "poly_rings", "ring_order")


def share(record, stats_csv):
    """The kernels' time per call from a rocprofv3 kernel_stats.csv of an `--only nest` run, per kernel and as a share of the calls' medians."""
    rec = json.load(open(record))
    calls = sum(s["nest_calls"] for s in rec["scenes"].values())
    per_call_ms = sum(s["ms"]["nest_alone"]["median"] * s["nest_calls"] for s in rec["scenes"].values()) / calls
    rows = list(csv.DictReader(open(stats_csv)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname"))
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    mine = {}
    for r in rows:
        m = re.search(r"k_nest_\w+", r[name])
        if m:
            mine[m.group(0)] = mine.get(m.group(0), 0.0) + float(r[total]) * 1e-6 / calls
    out = {"calls": calls, "entry_ms_per_call": per_call_ms, "kernel_ms_per_call": sum(mine.values()), "kernel_share": sum(mine.values()) / per_call_ms,
           "kernels_ms_per_call": dict(sorted(mine.items(), key=lambda kv: -kv[1]))}
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("nest",), default=None)
    ap.add_argument("--share", nargs=2, metavar=("RECORD", "KERNEL_STATS_CSV"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_nest_ab.json"))
    args = ap.parse_args()
    if args.share:
        return share(*args.share)
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")

    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
    odet, omask, _n_objects = objects_scene(tiles, 100)
    united = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    bdet, bmask, bsizes = batch_scene()
    encoded = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
    scenes = {"tiled": (united[3], [(H_IMG, W_IMG)]), "batch": (encoded[1], bsizes)}
    rec = {"git": git_head(), "steps": args.steps, "warmup": args.warmup, "only": args.only, "scenes": {}}
    ok = True
    for name, (rles, sizes) in scenes.items():
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())
        traced = D.rle_to_polygons(pair, sizes, flat=True)
        torch.cuda.synchronize()

        def device():
            out = D.rle_to_polygons(pair, sizes, flat=True, nest=True)
            torch.cuda.synchronize()
            return out["nest"]

        def nest_alone():
            out = D.nest_polygons(traced)
            torch.cuda.synchronize()
            return out

        def host():
            t = D.rle_to_polygons(pair, sizes, flat=True)
            return D.nest_polygons_host({k: t[k].cpu().numpy() for k in ("rle_rings", "ring_offsets", "xy")})
        got = nest_alone()
        calls, same = 1, None
        if not args.only:
            want = host()
            same = bool(all(np.array_equal(g[k].cpu().numpy().reshape(-1), want[k].reshape(-1)) for g in (got, device()) for k in KEYS)
                        and got["n_polys"] == want["n_polys"])
            ok = ok and same
        legs = (("nest_alone", nest_alone),) if args.only else (("device", device), ("nest_alone", nest_alone), ("host", host))
        times = {k: [] for k, _ in legs}
        for step in range(args.warmup + args.steps):
            for k, leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                if step >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
            calls += 1
        depth = got["depth"].cpu().numpy()
        per_rle = np.diff(traced["rle_rings"].cpu().numpy())
        ms = {k: stats(v) for k, v in times.items()}
        scene = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "rings": traced["n_rings"], "vertices": traced["n_vertices"],
                 "polygons": got["n_polys"], "holes": int((depth % 2 == 1).sum()), "deepest": int(depth.max()) if depth.size else 0,
                 "most_rings_in_one_rle": int(per_rle.max()), "arrays_equal": same, "nest_calls": calls, "ms": ms}
        if not args.only:
            scene["host_over_device"] = ms["host"]["median"] / ms["device"]["median"]
        rec["scenes"][name] = scene
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
