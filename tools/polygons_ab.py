"""Polygons out: what mrcnn_rle_to_polygons costs against the route a host had before, in one process on the GPU.

  polygons_ab.py [--steps 20] [--warmup 3] [--only device] [--out profiles/polygons_ab.json]
  polygons_ab.py --share profiles/polygons_ab.json <kernel_stats.csv>

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  legs    device   detection.rle_to_polygons on the device-resident (counts, run_offsets) pair, the rings left on the device: the whole
                   entry with its binding — prefix pass, count, the summary read back, trace, the rings read back, write.  The binding's
                   first guess of the two capacities holds in both scenes, so a call is one call of the entry
          host     the only route before: the runs copied to the host, the sequential definition (mrcnn_rle_to_polygons_host: decode
                   every plane, walk its edges), the result kept on the host

Before anything is timed the device result is compared with the host definition's, array by array.  The legs alternate inside every
step; every figure is the median of --steps calls after --warmup untimed ones, with min and max beside it, taken with a host clock
around calls that end synchronised.  The kernels' share of a device call comes from a second run: `rocprofv3 --kernel-trace --stats`
around `polygons_ab.py --only device`, whose kernel_stats.csv `--share` divides by that run's calls and medians (kernels k_rle_prefix and
k_polygon_*).  No time was promised for either route; the result says which leg won."""
import argparse, csv, importlib, json, os, re, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

KEYS = ("rle_rings", "ring_offsets", "ring_areas", "xy")


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
        m = re.search(r"k_polygon_\w+|k_rle_prefix", r[name])
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
    ap.add_argument("--only", choices=("device",), default=None)
    ap.add_argument("--share", nargs=2, metavar=("RECORD", "KERNEL_STATS_CSV"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_ab.json"))
    args = ap.parse_args()
    if args.share:
        return share(*args.share)
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    limit = importlib.import_module("mask-rcnn-coreml_amd._lib").POLYGON_LDS_CORNERS

    tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
    odet, omask, n_objects = objects_scene(tiles, 100)
    united = D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)
    bdet, bmask, bsizes = batch_scene()
    encoded = D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)
    scenes = {"tiled": (united[3], [(H_IMG, W_IMG)], {"objects": n_objects, "components": int(united[2][0])}), "batch": (encoded[1], bsizes, {})}
    rec = {"git": git_head(), "steps": args.steps, "warmup": args.warmup, "only": args.only, "scenes": {}}
    ok = True
    for name, (rles, sizes, extra) in scenes.items():
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())

        def device():
            out = D.rle_to_polygons(pair, sizes, flat=True)
            torch.cuda.synchronize()
            return out

        def host():
            return D.rle_to_polygons_host((pair[0].cpu().numpy().view(np.uint32), pair[1].cpu().numpy()), sizes, flat=True)
        got = device()
        calls = 1
        same = None
        if not args.only:
            want = host()
            same = bool(all(np.array_equal(got[k].cpu().numpy().reshape(-1), want[k].reshape(-1)) for k in KEYS))
            ok = ok and same
        legs = (("device", device),) if args.only else (("device", device), ("host", host))
        times = {k: [] for k, _ in legs}
        for step in range(args.warmup + args.steps):
            for k, leg in legs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                if step >= args.warmup:
                    times[k].append(time.perf_counter() - t0)
            calls += 1
        ro, rr = got["ring_offsets"].cpu().numpy(), got["rle_rings"].cpu().numpy()
        corners = ro[rr[1:]] - ro[rr[:-1]]
        ms = {k: stats(v) for k, v in times.items()}
        rec["scenes"][name] = dict(extra, images=len(sizes), size=list(sizes[0]), slots=len(rles[0]), runs=int(counts.size), rings=got["n_rings"],
                                   vertices=got["n_vertices"], holes=int((got["ring_areas"] < 0).sum().item()), most_corners=int(corners.max()),
                                   rles_above_the_lds_limit=int((corners > limit).sum()), arrays_equal=same, device_calls=calls, ms=ms,
                                   algorithmic_bytes=int(4 * counts.size + 8 * got["n_vertices"] + 16 * got["n_rings"]))
        if not args.only:
            rec["scenes"][name]["device_over_host"] = ms["host"]["median"] / ms["device"]["median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
