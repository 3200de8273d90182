"""COCOeval's accumulate: numpy on the host against mrcnn_coco_accumulate on the device, in one process, on synthetic records.

  coco_accumulate_ab.py [--images 1000 5000] [--seed 11] [--warmup 1] [--repeats 5] [--out profiles/coco_accumulate_ab.txt]

The records (seeded, no dataset ships here) have COCO's shape: 80 categories, 100 detections per image, 4 area ranges x 10 IoU thresholds
of matched / ignore flags, 7 ground truths per image on average.  A quarter of the detections fall into category 0 (a long segment, as
"person" is one), the rest evenly over the others; scores are float32 values quantised to 1 / 256, so ties are frequent.
    A   coco_eval.accumulate(evals)                       numpy and Python on one host thread: the definition
    B   coco_eval.accumulate_device(evals, device=None)   pack_evals, then mrcnn_coco_accumulate over host arrays: the library uploads
        the tables and downloads the two results — what score() runs with accumulate_on="device"
    C   coco_eval.accumulate_device(evals, device="cuda") the same with the tables uploaded as torch tensors and read in place
Every leg starts from the same records and ends with numpy arrays on the host, so packing and transfers are inside the window.  The three
results are compared bit for bit before anything is timed.  `--warmup` untimed calls, then the median of `--repeats`, per leg."""
import argparse, importlib, os, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, A, T, ROWS = 80, 4, 10, 100


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def synthetic_records(n_images, seed):
    rng = np.random.default_rng(seed)
    p_cat = np.full(K, 0.75 / (K - 1)); p_cat[0] = 0.25
    evals = [[] for _ in range(K)]
    for _ in range(n_images):
        cats = rng.choice(K, ROWS, p=p_cat)
        scores = (np.ceil(rng.random(ROWS).astype(np.float32) * 256) / 256).astype(np.float64)
        gt_cats = rng.choice(K, int(rng.poisson(7.0)), p=p_cat)
        for k in np.union1d(cats, gt_cats):
            s = np.sort(scores[cats == k])[::-1]
            nd, ng = s.size, int((gt_cats == k).sum())
            matched = rng.random((A, T, nd)) < np.linspace(0.6, 0.2, T)[None, :, None] * (ng > 0)
            evals[k].append({"scores": s, "matched": matched, "ignore": rng.random((A, T, nd)) < 0.1, "gt_ignore": rng.random((A, ng)) < 0.3})
    return evals


def median_ms(fn, warmup, repeats, sync):
    ts = []
    for step in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if step >= warmup:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[0] * 1e3, ts[len(ts) // 2] * 1e3, ts[-1] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_accumulate_ab.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("coco_accumulate_ab.py measures on the GPU: no device")          # never a CPU figure in its place
    CE = importlib.import_module("mask-rcnn-coreml_amd.coco_eval")
    lines = [f"git_head {git_head()}", f"device {torch.cuda.get_device_name(0)}"]

    def say(line):
        lines.append(line)
        print(line, flush=True)
    for line in lines:
        print(line, flush=True)
    for n_images in args.images:
        evals = synthetic_records(n_images, args.seed)
        P = CE.pack_evals(evals)
        n = P["scores"].size
        say(f"set: seed {args.seed}, {n_images} images, {K} categories, {sum(len(E) for E in evals)} records, {n} detections, the longest category "
            f"{int(np.diff(P['cat_offsets']).max())}, {np.unique(P['scores']).size} distinct scores, flags {A} x {T} planes")
        a = CE.accumulate(evals)
        b = CE.accumulate_device(evals, device=None)
        c = CE.accumulate_device(evals, device="cuda")
        assert all(np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]) for i in (0, 1)), "the legs disagree"
        say(f"agreement: precision {a[0].shape} and recall {a[1].shape}, bit for bit, {int((a[0] > 0).sum())} positive entries")
        a0, a1, a2 = median_ms(lambda: CE.accumulate(evals), args.warmup, args.repeats, lambda: None)
        say(f"A host, accumulate                           ms min/median/max  {a0:.1f} / {a1:.1f} / {a2:.1f}")
        b0, b1, b2 = median_ms(lambda: CE.accumulate_device(evals, device=None), args.warmup, args.repeats, torch.cuda.synchronize)
        say(f"B device, accumulate_device(device=None)     ms min/median/max  {b0:.1f} / {b1:.1f} / {b2:.1f}")
        c0, c1, c2 = median_ms(lambda: CE.accumulate_device(evals, device="cuda"), args.warmup, args.repeats, torch.cuda.synchronize)
        say(f"C device, accumulate_device(device='cuda')   ms min/median/max  {c0:.1f} / {c1:.1f} / {c2:.1f}")
        p0, p1, p2 = median_ms(lambda: CE.pack_evals(evals), args.warmup, args.repeats, lambda: None)
        say(f"  of B and C: pack_evals alone               ms min/median/max  {p0:.1f} / {p1:.1f} / {p2:.1f}")
        say(f"A / B (medians) {a1 / b1:.2f}, A / C {a1 / c1:.2f}; warm-up calls {args.warmup}, timed calls {args.repeats} per leg")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
