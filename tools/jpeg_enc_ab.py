"""JPEG files out: what it costs to get eight rendered pictures off the device as files, in one process on the GPU.

  jpeg_enc_ab.py [--steps 20] [--warmup 3] [--seed 3] [--out profiles/jpeg_enc_ab.json]
  jpeg_enc_ab.py --kernels-only                  a few calls of leg B and nothing else: the program to put behind
                                                 rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
  jpeg_enc_ab.py --digest DIR [--out FILE]       per-kernel microseconds from that run's *kernel_stats.csv, merged into FILE

The workload: eight 640x480 pictures rendered by mrcnn_render_detections_source (a small synthetic model's detections drawn over
smooth seeded scenes plus noise), resident on the device as the render left them; quality 90, 4:2:0.

  A  what a host could do before this entry existed: the device-to-host copy of the RGB (3*h*w bytes per picture), then PIL's encoder
     (libjpeg-turbo) on one thread where PIL imports — otherwise mrcnn_jpeg_encode_host, and the result says which it was
  B  jpeg.encode_batch on the device tensors (mrcnn_jpeg_encode_batch): only the files cross back

Before anything is timed B's files are compared byte for byte with mrcnn_jpeg_encode_host's, and — with PIL — their decoded pixels
with the decoded pixels of PIL's own files.  A and B alternate inside every step; every figure is the median of --steps calls after
--warmup untimed ones, with min and max beside it.  The bar: B's median below A's by more than A's own min-to-max spread."""
import argparse, csv, glob, importlib, io, json, os, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, H, W, QUALITY = 8, 480, 640, 90


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def stats(ts, images):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"images_per_s": images / med, "ms": {"min": ts[0] * 1e3, "median": med * 1e3, "max": ts[-1] * 1e3}}


def rendered_on_device(seed):
    import torch
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(128, 128, 3), num_classes=21, pre_nms_max_proposals=300, max_proposals=64,
                          max_detections=16)
    mdir = tempfile.mkdtemp(prefix="mrcnn_jpeg_enc_")
    weights.save_synthetic_models(mdir, cfg, seed=0)
    m = models.load_maskrcnn(mdir, max_batch=BATCH)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    images = []
    for b in range(BATCH):
        base = [128 + 100 * np.sin(xx / (23.0 + 3 * b) + c) * np.cos(yy / (31.0 + 2 * c)) for c in range(3)]
        images.append(torch.from_numpy(np.clip(np.stack(base, -1) + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)).cuda())
    out = m.render_images(images, min_score=0.0)
    torch.cuda.synchronize()
    drawn = sum(int((o != i).any(-1).sum()) for o, i in zip(out, images))
    return out, drawn


def digest(directory):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                r = {k.lower(): v for k, v in r.items() if k}
                name = r.get("name") or r.get("kernelname") or ""
                if "k_jpeg_" in name or "fill" in name.lower():
                    short = name.split("(")[0].split("::")[-1].split("<")[0]
                    rows[short] = {"calls": int(r["calls"]), "average_us": float(r["averagens"]) / 1e3, "total_us": float(r["totaldurationns"]) / 1e3}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--digest", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.digest:
        res = {}
        if args.out and os.path.exists(args.out):
            with open(args.out) as f:
                res = json.load(f)
        res["kernels"] = digest(args.digest)
        res["kernels_sum_of_averages_us"] = sum(v["average_us"] for k, v in res["kernels"].items() if k.startswith("k_jpeg_") and "idct" not in k and "color" not in k)
        text = json.dumps(res, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return

    import torch
    assert torch.cuda.is_available(), "jpeg_enc_ab.py measures on the GPU: there is no fallback"
    J = importlib.import_module("mask-rcnn-coreml_amd.jpeg")
    images, drawn = rendered_on_device(args.seed)
    if args.kernels_only:
        for _ in range(5):
            J.encode_batch(images, QUALITY, "420")
        return
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def leg_a():
        host = [im.cpu().numpy() for im in images]
        if Image is None:
            return [J.encode_host(h, QUALITY, "420") for h in host]
        files = []
        for h in host:
            bio = io.BytesIO()
            Image.fromarray(h).save(bio, "JPEG", quality=QUALITY, subsampling=2)
            files.append(bio.getvalue())
        return files

    def leg_b():
        return J.encode_batch(images, QUALITY, "420")

    # equality first
    host = [im.cpu().numpy() for im in images]
    a, b = leg_a(), leg_b()
    assert b == [J.encode_host(h, QUALITY, "420") for h in host], "encode_batch differs from encode_host"
    if Image is not None:
        for fa, fb in zip(a, b):
            assert np.array_equal(np.array(Image.open(io.BytesIO(fa)).convert("RGB")), J.decode_host(fb)), "our file decodes to other pixels than PIL's"
    res = {"git_head": git_head(), "workload": f"eight rendered {W}x{H} pictures on the device, q{QUALITY} 4:2:0, {drawn} drawn pixels",
           "leg_A_encoder": "PIL (libjpeg-turbo), one thread" if Image is not None else "mrcnn_jpeg_encode_host (no PIL here)",
           "steps": args.steps, "warmup": args.warmup, "file_bytes_B": [len(f) for f in b], "file_bytes_A": [len(f) for f in a],
           "pcie_bytes_A": sum(int(im.numel()) for im in images), "pcie_bytes_B": sum(len(f) for f in b) + 8 * (BATCH + 1)}
    times = {"A": [], "B": []}
    for step in range(args.warmup + args.steps):
        for k, leg in (("A", leg_a), ("B", leg_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                times[k].append(dt)
    res["A_copy_then_host_encoder"] = stats(times["A"], BATCH)
    res["B_encode_batch"] = stats(times["B"], BATCH)
    am, bm = res["A_copy_then_host_encoder"]["ms"], res["B_encode_batch"]["ms"]
    res["A_spread_ms"] = am["max"] - am["min"]
    res["bar_B_median_below_A_median_by_more_than_A_spread"] = bool(am["median"] - bm["median"] > res["A_spread_ms"])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
