"""PNG files out: what it costs to get eight instance maps off the device as files, in one process on the GPU.

  png_ab.py [--steps 30] [--warmup 5] [--seed 3] [--out profiles/png_ab.json]

The workload: eight 640x480 int16 instance maps as mrcnn_instance_map_source leaves them on the device (24 synthetic detections an
image, smooth blob masks stretched over random boxes), written as MRCNN_PNG_INSTANCE files with rows = 24.

  A  what a host could do before this entry existed: the device-to-host copy of the maps (2*h*w bytes an image), then on one core
     the index bytes and filter bytes in numpy, zlib.compress at level 6, and the chunks with zlib.crc32
  B  png.encode_batch on the device tensors (mrcnn_png_encode_batch): only the files cross back

Before anything is timed B's files are compared byte for byte with mrcnn_png_encode_host's, and both legs' files are parsed back to
the maps.  A and B alternate inside every step; every figure is the median of --steps calls after --warmup untimed ones, with min
and max beside it, taken with a host clock around work that ends synchronised (both legs end in a device-to-host copy).  The sizes
of the files are reported side by side: B's matcher sees distance 1 only and its Huffman codes are fixed, so zlib's files are
smaller.  No speed-up was promised for B; the result says which leg won."""
import argparse, importlib, json, os, struct, subprocess, sys, time, zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, H, W, ROWS, MODEL = 8, 480, 640, 24, 1024
PALETTE = ((255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0))


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def stats(ts, images):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"images_per_s": images / med, "ms": {"min": ts[0] * 1e3, "median": med * 1e3, "max": ts[-1] * 1e3}}


def maps_on_device(seed):
    """Eight maps from mrcnn_instance_map_source on CUDA tensors: the buffers the encoder reads in place."""
    import torch
    D = importlib.import_module("mask-rcnn-coreml_amd.detection")
    rng = np.random.default_rng(seed)
    det = np.zeros((BATCH, ROWS, 6), np.float32)
    masks = np.zeros((BATCH, ROWS, 28, 28), np.float32)
    yy, xx = np.mgrid[0:28, 0:28].astype(np.float32)
    for b in range(BATCH):
        y1, x1 = rng.random(ROWS) * 0.7, rng.random(ROWS) * 0.7
        det[b, :, 0], det[b, :, 1] = y1, x1
        det[b, :, 2], det[b, :, 3] = np.minimum(1.0, y1 + 0.05 + rng.random(ROWS) * 0.3), np.minimum(1.0, x1 + 0.05 + rng.random(ROWS) * 0.3)
        det[b, :, 4] = rng.integers(1, 80, ROWS)
        det[b, :, 5] = np.linspace(0.99, 0.35, ROWS)
        for i in range(ROWS):
            cy, cx, sy, sx = rng.uniform(10, 18), rng.uniform(10, 18), rng.uniform(5, 10), rng.uniform(5, 10)
            masks[b, i] = np.exp(-(((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2))
    _, maps, _ = D.instance_map_source(torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), [(H, W)] * BATCH, MODEL, MODEL, 0.5, 0.0)
    torch.cuda.synchronize()
    return maps


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def host_png(m):
    """Leg A's encoder: the same file format, zlib's level 6 stream."""
    idx = np.where((m >= -1) & (m < ROWS), m + 1, 0).astype(np.uint8)
    raw = np.concatenate([np.zeros((m.shape[0], 1), np.uint8), idx], axis=1).tobytes()
    plte = bytes(3) + b"".join(bytes(PALETTE[(k - 1) % 4]) for k in range(1, ROWS + 1))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", m.shape[1], m.shape[0], 8, 3, 0, 0, 0)) + chunk(b"PLTE", plte) + chunk(b"tRNS", b"\0") +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "png_ab.py measures on the GPU: there is no fallback"
    P = importlib.import_module("mask-rcnn-coreml_amd.png")
    maps = maps_on_device(args.seed)

    def leg_a():
        return [host_png(m.cpu().numpy()) for m in maps]

    def leg_b():
        return P.encode_batch(maps, rows=ROWS)

    # equality first
    host = [m.cpu().numpy() for m in maps]
    a, b = leg_a(), leg_b()
    assert b == [P.encode_host(h, ROWS) for h in host], "encode_batch differs from encode_host"
    for fa, fb, h in zip(a, b, host):
        for f in (fa, fb):
            assert np.array_equal(P.parse(f)["scanlines"].astype(np.int16) - 1, h), "a file does not parse back to its map"
    owned = sum(int((h >= 0).sum()) for h in host)
    res = {"git_head": git_head(), "workload": f"eight {W}x{H} int16 instance maps on the device, {ROWS} rows, {owned} owned pixels of {BATCH * H * W}",
           "leg_A_encoder": "device-to-host copy of the maps, numpy index bytes, zlib.compress level 6, zlib.crc32 framing, one core",
           "steps": args.steps, "warmup": args.warmup, "raw_stream_bytes_per_image": H * (W + 1),
           "file_bytes_B": [len(f) for f in b], "file_bytes_A": [len(f) for f in a],
           "file_bytes_B_over_A": sum(len(f) for f in b) / sum(len(f) for f in a),
           "pcie_bytes_A": sum(int(m.numel()) * 2 for m in maps), "pcie_bytes_B": sum(len(f) for f in b) + 8 * (BATCH + 1)}
    times = {"A": [], "B": []}
    for step in range(args.warmup + args.steps):
        for k, leg in (("A", leg_a), ("B", leg_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            dt = time.perf_counter() - t0
            if step >= args.warmup:
                times[k].append(dt)
    res["A_copy_then_zlib6"] = stats(times["A"], BATCH)
    res["B_encode_batch"] = stats(times["B"], BATCH)
    am, bm = res["A_copy_then_zlib6"]["ms"], res["B_encode_batch"]["ms"]
    res["A_spread_ms"] = am["max"] - am["min"]
    res["B_median_below_A_median_by_more_than_A_spread"] = bool(am["median"] - bm["median"] > res["A_spread_ms"])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
