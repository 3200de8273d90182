"""Writes tests/golden/jpeg_enc_v1.npz: small source images and, for each, the RGB that PIL decodes from PIL's OWN encoding of it
(libjpeg-turbo's default compressor: save(quality=q, subsampling=s, optimize=False)).  The project's decoder is pinned to libjpeg byte
for byte (jpeg_v1.npz), so decode_host(encode_host(pixels)) == ref_rgb compares the encoder's coefficients and tables with libjpeg's
on every visible sample.  The only new place that imports PIL; the tests read the .npz.  Needs the built library (encode_host).

    python tests/golden/make_jpeg_enc_golden.py

Per case NAME the file holds NAME_pixels ((h, w, 3) uint8; R = G = B for a grey case), NAME_params = [quality, sampling] (sampling:
0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, 3 = grey, PIL mode L) and NAME_ref ((h, w, 3) uint8).  The generator also encodes every case with
encode_host, walks the scans and asserts that the set exercises byte stuffing (FF 00), ZRL codes and a final padded byte of FF."""
import importlib
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_jpeg_golden import synthetic  # noqa: E402

# name: (height, width, quality, sampling, kind)
CASES = [
    ("one_pixel", 1, 1, 75, 2, "synthetic"),
    ("one_block", 8, 8, 75, 0, "synthetic"),
    ("one_over", 9, 9, 75, 0, "synthetic"),
    ("exact_mcu", 16, 16, 75, 2, "synthetic"),
    ("odd_444", 17, 23, 90, 0, "synthetic"),
    ("odd_422", 33, 47, 75, 1, "synthetic"),
    ("odd_420", 35, 45, 75, 2, "synthetic"),
    ("even_420", 22, 26, 75, 2, "synthetic"),       # an even height that is no multiple of 16: the rows below repeat a chroma ROW
    ("narrow", 31, 9, 100, 2, "synthetic"),
    ("coarse", 40, 40, 3, 2, "synthetic"),
    ("grey", 40, 40, 75, 3, "synthetic"),
    ("saturated", 24, 24, 100, 0, "saturated"),     # uniform noise at q100: the largest size categories, every clamp
    ("flat", 32, 32, 75, 2, "flat"),                # every block is DC + EOB
    ("zrl", 32, 32, 50, 0, "zrl"),                  # one high-frequency term per block: runs of >= 16 zeros
    ("pad_ff", 8, 8, 75, 0, "search"),              # the scan's last byte, padding included, is FF (and is stuffed)
]


def pixels_of(name, h, w, sampling, kind, rng):
    if kind == "flat":
        return np.broadcast_to(np.array([200, 120, 40], np.uint8), (h, w, 3)).copy()
    if kind == "zrl":
        yy, xx = np.mgrid[0:8, 0:8]
        img = np.zeros((h, w), np.float64)
        for by in range(h // 8):
            for bx in range(w // 8):
                u, v = 7 - (bx % 3), 7 - (by % 3)              # (7,7) is zigzag 63: a run of 62 zeros, three ZRLs
                img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = 128 + 100 * np.cos((2 * xx + 1) * u * np.pi / 16) * np.cos((2 * yy + 1) * v * np.pi / 16)
        g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
        return np.stack([g] * 3, -1)
    img = synthetic(name, h, w, "L" if sampling == 3 else "RGB", rng)
    return np.stack([img] * 3, -1) if sampling == 3 else img


def pil_reference(pixels, quality, sampling):
    bio = io.BytesIO()
    if sampling == 3:
        Image.fromarray(np.ascontiguousarray(pixels[..., 0]), "L").save(bio, "JPEG", quality=quality, optimize=False)
    else:
        Image.fromarray(pixels, "RGB").save(bio, "JPEG", quality=quality, subsampling=sampling, optimize=False)
    return bio.getvalue(), np.array(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))


def segments(data):
    """{marker: [payload, ...]} of the segments up to SOS, and the offset of the scan's first byte."""
    out, pos = {}, 2
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        out.setdefault(m, []).append(data[pos + 4:pos + 2 + n])
        pos += 2 + n
        if m == 0xDA:
            return out, pos


def huffman_tables(segs):
    """{(class, id): {(length, code): symbol}} from the DHT segments."""
    tables = {}
    for seg in segs[0xC4]:
        i = 0
        while i < len(seg):
            key, bits = (seg[i] >> 4, seg[i] & 15), seg[i + 1:i + 17]
            vals, code, k, t = seg[i + 17:i + 17 + sum(bits)], 0, 0, {}
            for length in range(1, 17):
                for _ in range(bits[length - 1]):
                    t[(length, code)] = vals[k]
                    k, code = k + 1, code + 1
                code <<= 1
            tables[key] = t
            i += 17 + sum(bits)
    return tables


def walk_scan(data):
    """Entropy-decodes a file written by encode_host far enough to count: (stuffed FF 00 pairs, ZRL codes, last scan byte)."""
    segs, start = segments(data)
    assert data[-2:] == b"\xff\xd9"
    scan = data[start:-2]
    stuffed = scan.count(b"\xff\x00")
    raw = scan.replace(b"\xff\x00", b"\xff")
    bits = "".join(f"{b:08b}" for b in raw)
    sof = segs[0xC0][0]
    h, w, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    hs, vs = (sof[7] >> 4, sof[7] & 15) if nc == 3 else (1, 1)
    tables = huffman_tables(segs)
    blocks = [0] * (hs * vs) + [1, 1] if nc == 3 else [0]
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    pos, zrl = 0, 0

    def symbol(t):
        nonlocal pos
        code = 0
        for length in range(1, 17):
            code = (code << 1) | int(bits[pos + length - 1])
            if (length, code) in t:
                pos += length
                return t[(length, code)]
        raise AssertionError("no such code")

    for _ in range(mcus):
        for tid in blocks:
            size = symbol(tables[(0, tid)])             # (symbol moves pos itself: read it only afterwards)
            pos += size
            k = 1
            while k < 64:
                rs = symbol(tables[(1, tid)])
                if rs == 0:
                    break
                if rs == 0xF0:
                    zrl += 1
                    k += 16
                    continue
                k += (rs >> 4) + 1
                pos += rs & 15
    assert len(bits) - pos < 8 and set(bits[pos:]) <= {"1"}, "the scan does not end in 1-padding"
    return stuffed, zrl, raw[-1]


def main():
    jpeg = importlib.import_module("mask-rcnn-coreml_amd.jpeg")
    rng = np.random.default_rng(20260101)
    out, counts = {}, {"stuffed": 0, "zrl": 0, "pad_ff": 0}
    for name, h, w, quality, sampling, kind in CASES:
        if kind == "search":
            pixels = None
            for seed in range(20000):
                cand = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
                data = jpeg.encode_host(cand, quality, sampling)
                if data[-4:] == b"\xff\x00\xff\xd9":
                    pixels = cand
                    print(f"{name}: seed {seed} ends its scan in a padded FF")
                    break
            assert pixels is not None, "no 8x8 image whose scan ends in FF among the seeds"
        else:
            pixels = pixels_of(name, h, w, sampling, kind, rng)
        pil_file, ref = pil_reference(pixels, quality, sampling)
        ours = jpeg.encode_host(pixels, quality, sampling)
        # the tables of the file are the standard ones: PIL (optimize=False) writes exactly those
        mine, theirs = segments(ours)[0], segments(pil_file)[0]
        assert b"".join(mine[0xC4]) == b"".join(theirs[0xC4]), f"{name}: the Huffman tables are not the standard ones"
        assert b"".join(mine[0xDB]) == b"".join(theirs[0xDB]), f"{name}: the quantisation tables differ from libjpeg's"
        stuffed, zrl, last = walk_scan(ours)
        counts["stuffed"] += stuffed
        counts["zrl"] += zrl
        counts["pad_ff"] += int(last == 0xFF)
        diff = int(np.abs(jpeg.decode_host(ours).astype(np.int32) - ref.astype(np.int32)).max())
        print(f"{name:10s} {h:3d}x{w:<3d} q{quality:<3d} sampling {sampling}: {len(ours):5d} bytes (PIL {len(pil_file):5d}), stuffed {stuffed}, ZRL {zrl}, "
              f"max |decode - PIL| = {diff}")
        out[name + "_pixels"] = pixels
        out[name + "_params"] = np.array([quality, sampling], np.int32)
        out[name + "_ref"] = ref
    print("over the set:", counts)
    assert counts["stuffed"] >= 1 and counts["zrl"] >= 1 and counts["pad_ff"] >= 1, counts
    path = os.path.join(HERE, "jpeg_enc_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; jpeg_v1.npz:", os.path.getsize(os.path.join(HERE, "jpeg_v1.npz")))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "jpeg_v1.npz"))


if __name__ == "__main__":
    main()
