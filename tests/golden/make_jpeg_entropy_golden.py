"""Writes tests/golden/jpeg_entropy_v1.npz: the JPEG files the tests of the device entropy stage add to jpeg_v1.npz's.  File bytes only
(NAME_jpg, uint8) — the expectation is the project's own host decoder — plus `large_seed`, the seed of the one larger file the tests
generate themselves.  Imports PIL (the encoder of the fixture files) and the package (jpeg.encode_host, for the seed search).

    python tests/golden/make_jpeg_entropy_golden.py

All images are 120x160 gradients plus seeded noise, as in make_jpeg_golden.py (noise of +-1, so that the four stay under 64 KB):
    restarts7   4:2:0 q90, restart_marker_blocks=7: 80 MCUs, 12 intervals — the marker number wraps past RST7, the last interval is short
    optimized   4:4:4 q98, optimize=True: the file's own Huffman tables, long codes
    h2v1        4:2:2 q95
    grey        one component, q90
and five FLAT images, whose scans and restart intervals end on blocks of a few bits (DC difference 0 + end of block = 6 bits with the
standard tables) — shorter than the padding in front of a marker can be:
    flat_grey       64x64 grey 128, q90                 flat_128 / flat_77       120x160 RGB of that value, 4:2:0 q75
    flat_128_rst / flat_77_rst   the same two with restart_marker_blocks=3
and two files in which a segment's last data byte is an FF, so that its stuffed 00 stands directly in front of the marker (a block that
ends on coefficient 63 with extra bits of ones, then the ones of the padding): uniform-noise RGB at q100 4:4:4, the first seed that gives
    tail_rst    16x16, restart_marker_blocks=1: holds FF 00 FF Dn, the FF closing a 4-byte unit          tail_eoi    8x8, no DRI: ends FF 00 FF D9
The larger file is NOT stored: tests build it from `large_image(large_seed)` with jpeg.encode_host(quality 90, "420") — 240x320, about
56 KB, more than one workgroup of production units.  The seed is the first from 20260201 on whose file holds a stuffed FF 00 whose FF is
the last byte of a 128-byte unit counted from the scan's first byte."""
import importlib
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
H, W = 120, 160
CASES = [
    ("restarts7", "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=7)),
    ("optimized", "RGB", dict(quality=98, subsampling=0, optimize=True)),
    ("h2v1", "RGB", dict(quality=95, subsampling=1)),
    ("grey", "L", dict(quality=90)),
]
# name: (height, width, mode, value, save options)
FLAT = [
    ("flat_grey", 64, 64, "L", 128, dict(quality=90)),
    ("flat_128", H, W, "RGB", 128, dict(quality=75, subsampling=2)),
    ("flat_77", H, W, "RGB", 77, dict(quality=75, subsampling=2)),
    ("flat_128_rst", H, W, "RGB", 128, dict(quality=75, subsampling=2, restart_marker_blocks=3)),
    ("flat_77_rst", H, W, "RGB", 77, dict(quality=75, subsampling=2, restart_marker_blocks=3)),
]


from make_jpeg_entropy_golden_images import large_image, synthetic            # (what the tests import too: numpy only)


def scan_start(data):
    pos = 2
    while True:
        assert data[pos] == 0xFF
        m, n = int(data[pos + 1]), (int(data[pos + 2]) << 8) | int(data[pos + 3])
        pos += 2 + n
        if m == 0xDA:
            return pos


def stuffed_tails(data):
    """For every segment of the scan whose last data byte is an FF (FF 00 directly in front of the marker): the offset of that FF from
    the segment's first byte."""
    s, out = scan_start(data), []
    b0 = i = s
    while i < len(data) - 1:
        if data[i] == 0xFF and data[i + 1] != 0x00:
            if i - b0 >= 2 and data[i - 2] == 0xFF and data[i - 1] == 0x00:
                out.append(i - 2 - b0)
            b0 = i = i + 2
        else:
            i += 2 if data[i] == 0xFF else 1
    return out


def stuffed_at_unit_end(data, unit):
    """Stuffed FF 00 pairs of the scan whose FF is the last byte of a `unit`-byte unit counted from the scan's first byte."""
    a = np.frombuffer(data, np.uint8)
    s = scan_start(a)
    ff = np.flatnonzero((a[s:-1] == 0xFF) & (a[s + 1:] == 0x00))
    return int((ff % unit == unit - 1).sum())


def main():
    rng = np.random.default_rng(20260201)
    out = {}
    for name, mode, opts in CASES:
        bio = io.BytesIO()
        Image.fromarray(synthetic(H, W, mode, rng, noise=1), mode).save(bio, "JPEG", **opts)
        data = bio.getvalue()
        assert (b"\xff\xdd" in data[:scan_start(data)]) == (name == "restarts7")
        out[name + "_jpg"] = np.frombuffer(data, np.uint8)
    for name, h, w, mode, value, opts in FLAT:
        bio = io.BytesIO()
        Image.fromarray(np.full((h, w) if mode == "L" else (h, w, 3), value, np.uint8), mode).save(bio, "JPEG", **opts)
        out[name + "_jpg"] = np.frombuffer(bio.getvalue(), np.uint8)
    # tail_rst: one of its tails is also the LAST byte of a 4-byte unit of its segment — the stuffed 00 then opens the segment's last unit alone
    for name, side, opts, want in (("tail_rst", 16, dict(restart_marker_blocks=1), lambda d: any(t % 4 == 3 for t in stuffed_tails(d)[:-1])),
                                   ("tail_eoi", 8, dict(), lambda d: d.endswith(b"\xff\x00\xff\xd9"))):
        for seed in range(1000):
            bio = io.BytesIO()
            noise = np.random.default_rng(seed).integers(0, 256, (side, side, 3), dtype=np.uint8)
            Image.fromarray(noise, "RGB").save(bio, "JPEG", quality=100, subsampling=0, **opts)
            data = bio.getvalue()
            if want(data):
                break
        else:
            raise SystemExit(name + ": no seed gives the tail")
        out[name + "_jpg"] = np.frombuffer(data, np.uint8)
    sys.path.insert(0, ROOT)
    jpeg = importlib.import_module("mask-rcnn-coreml_amd.jpeg")
    seed = 20260201
    while True:
        data = jpeg.encode_host(large_image(seed), 90, "420")
        if stuffed_at_unit_end(data, 128) >= 1:
            break
        seed += 1
    out["large_seed"] = np.array([seed], np.int64)
    path = os.path.join(HERE, "jpeg_entropy_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: v.size for k, v in out.items() if k.endswith("_jpg")}, "large:", len(data), "bytes, seed", seed)


if __name__ == "__main__":
    main()
