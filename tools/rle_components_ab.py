"""Connected components of run-length masks: what mrcnn_rle_components and mrcnn_rle_components_select cost on device-resident runs
against the route a host has without them, in one process on the GPU.

  rle_components_ab.py [--steps 20] [--warmup 3] [--host-steps 1] [--only device] [--out profiles/rle_components_ab.json]
  rle_components_ab.py --share profiles/rle_components_ab_only.json <kernel_stats.csv>

  scenes  tiled    tools/tiled_ab.py's 4096x3072 scene of 60 synthetic objects larger than the overlap, united (mrcnn_unite_tiles): one
                   image, 100 slots
          batch    eight 640x480 images, 100 rows each, the RLEs of mrcnn_masks_rle_source (tools/rle_draw_ab.py's batch)
  work    components      detection.rle_components (ones, connectivity 4)
          remove_small    detection.rle_remove_small(min_area = 64): label, keep mask, MERGE
          fill_holes      detection.rle_fill_holes: label the zeros, keep mask, MERGE
          split           detection.rle_split_components: label, keep mask, SPLIT (the sort)
  legs    device   on the device-resident (counts, run_offsets) pair: measures, keep masks and results stay on the device
          host     the route a host has without the entries: the runs copied down, the sequential definitions there (a plane per RLE,
                   flooded), the result copied back to the device.  The definitions are written to be read, not to be fast (the
                   selection labels every plane twice): the ratio says what the entries save a host that has nothing else, not how
                   they compare with an optimised host labeller.  Seconds to minutes per call on the large scene: the first call is
                   timed (no warm-up), and --host-steps - 1 more only if that first call took under 20 s

Before anything is timed every device result is compared with the host definition's, array by array.  Every figure is the median of
the timed calls after --warmup untimed ones, with min and max beside it, taken with a host clock around calls that end synchronised.
The kernels' share of a call comes from a second run: `rocprofv3 --kernel-trace --stats --output-format csv` around
`rle_components_ab.py --only device`, which runs nothing but the four helpers in a row — once for the scene's figures, then the
warm-up and the timed steps — and counts those runs as it makes them; `--share` divides the k_cc_* kernels' total time in
kernel_stats.csv by that count and compares it with the mean of the timed four-in-a-row calls (k_rle_prefix and k_poly_scan, which
the scenes' own preparation launches too, are left out: under 0.3 ms a call together).  There is no pass bar; the result says which leg won and is written down as it is."""
import argparse, csv, importlib, json, os, re, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("MRCNN_TEST_KNOBS", "1")

from rle_draw_ab import batch_scene  # noqa: E402
from tiled_ab import H_IMG, MODEL, W_IMG, git_head, objects_scene, stats  # noqa: E402

MIN_AREA = 64
WORK = ("components", "remove_small", "fill_holes", "split")


def share(record, stats_csv):
    """The kernels' time per call from a rocprofv3 kernel_stats.csv of an `--only device` run, per kernel and as a share of the calls' medians."""
    rec = json.load(open(record))
    assert rec["only"] == "device", "the share needs the record of an --only device run: that run makes nothing but counted four-in-a-row calls"
    calls = sum(s["device_calls"] for s in rec["scenes"].values())
    per_call_ms = sum(s["ms"]["device"]["all"]["median"] * s["device_calls"] for s in rec["scenes"].values()) / calls
    rows = list(csv.DictReader(open(stats_csv)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname"))
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    mine = {}
    for r in rows:
        m = re.search(r"k_cc_\w+", r[name])
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


def flat(result):
    """every array of a result, on the host, uint32 where it is four bytes wide"""
    out = []
    for a in result:
        if isinstance(a, tuple):
            out += flat(a)
        else:
            a = a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)
            out.append(a.view(np.uint32) if a.dtype.itemsize == 4 else a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--only", choices=("device",), default=None)
    ap.add_argument("--scenes", default="tiled,batch")
    ap.add_argument("--git", default=None, help="the commit the record belongs to, where the tree that runs has no history of its own")
    ap.add_argument("--share", nargs=2, metavar=("RECORD", "KERNEL_STATS_CSV"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_components_ab.json"))
    args = ap.parse_args()
    if args.share:
        return share(*args.share)
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")

    scenes = {}
    if "tiled" in args.scenes:
        tiles = D.tile_plan(H_IMG, W_IMG, (MODEL, MODEL), (128, 128))
        odet, omask, _n_objects = objects_scene(tiles, 100)
        scenes["tiled"] = (D.unite_tiles(odet, omask, tiles, [(H_IMG, W_IMG)], MODEL, MODEL, 0.5, "iou", 0.5, None)[3], [(H_IMG, W_IMG)])
    if "batch" in args.scenes:
        bdet, bmask, bsizes = batch_scene()
        scenes["batch"] = (D.masks_rle_source(bdet, bmask, bsizes, MODEL, MODEL, 0.5)[1], bsizes)
    rec = {"git": args.git or git_head(), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "only": args.only, "min_area": MIN_AREA, "scenes": {}}
    ok = True
    for name, (rles, sizes) in scenes.items():
        counts = np.concatenate([r["counts"] for row in rles for r in row]).astype(np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(r["counts"]) for row in rles for r in row]))).astype(np.int64)
        pair = (torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(offs).cuda())
        torch.cuda.synchronize()
        device = {"components": lambda: D.rle_components(pair, sizes), "remove_small": lambda: D.rle_remove_small(pair, sizes, MIN_AREA),
                  "fill_holes": lambda: D.rle_fill_holes(pair, sizes), "split": lambda: D.rle_split_components(pair, sizes, MIN_AREA)}
        runs = {w: 0 for w in WORK}                              # how often each helper really ran on the device: --share divides by it

        def run(w):
            runs[w] += 1
            return device[w]()

        def down():
            return pair[0].cpu().numpy().view(np.uint32), pair[1].cpu().numpy()

        def up(result):
            return [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in flat(result)]
        host = {"components": lambda: up(D.rle_components_host(down(), sizes)), "remove_small": lambda: up(D.rle_remove_small_host(down(), sizes, MIN_AREA)),
                "fill_holes": lambda: up(D.rle_fill_holes_host(down(), sizes)), "split": lambda: up(D.rle_split_components_host(down(), sizes, MIN_AREA))}
        ms = {"device": {}, "host": {}}
        same, host_calls = {}, {}
        got = {w: run(w) for w in WORK}
        if not args.only:
            for w in WORK:
                t0 = time.perf_counter()
                want = host[w]()
                first = time.perf_counter() - t0
                same[w] = all(np.array_equal(g, h.cpu().numpy().view(g.dtype)) for g, h in zip(flat(got[w]), want)) and len(flat(got[w])) == len(want)
                ok = ok and same[w]
                more = timed(host[w], 0, args.host_steps - 1) if args.host_steps > 1 and first < 20.0 else []
                ms["host"][w] = stats([first] + more)
                host_calls[w] = 1 + len(more)
        if not args.only:                                        # (the profiled run makes four-in-a-row calls only)
            for w in WORK:
                ms["device"][w] = stats(timed(lambda: run(w), args.warmup, args.steps))
        ms["device"]["all"] = stats(timed(lambda: [run(w) for w in WORK], args.warmup, args.steps))
        assert len(set(runs.values())) == 1
        comp = flat(got["components"])
        scene = {"images": len(sizes), "size": list(sizes[0]), "slots": len(rles[0]), "runs_in": int(counts.size), "components": int(comp[0][-1]),
                 "components_below_min_area": int((comp[1] < MIN_AREA).sum()), "split_outputs": int(flat(got["split"])[2].shape[0]),
                 "plane_bytes_a_host_decodes": int(sum(h * w for h, w in sizes) * len(rles[0])), "arrays_equal": same or None,
                 "device_calls": runs[WORK[0]], "host_calls": {w: len_ for w, len_ in host_calls.items()} if not args.only else None, "ms": ms}
        if not args.only:
            ms["host"]["all"] = {"sum_of_medians": sum(ms["host"][w]["median"] for w in WORK)}
            scene["host_over_device"] = {w: ms["host"][w]["median"] / ms["device"][w]["median"] for w in WORK}
            scene["host_over_device"]["all"] = ms["host"]["all"]["sum_of_medians"] / ms["device"]["all"]["median"]
        rec["scenes"][name] = scene
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
