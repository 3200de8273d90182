"""Writes tests/golden/png_v1.npz: the PNG encoder's cases — samples in, the expected file's bytes out.

The bytes come from the sequential restatement of the format below, written from the format's description (include/maskrcnn_hip.h,
"PNG: files out") and RFC 1951 / the PNG specification, not from the C++: a greedy parse one token after another, the length codes
from RFC 1951's table as it is printed, a bit writer, zlib.adler32 and zlib.crc32.  Every file is checked with zlib.decompress
before it is stored.

    python tests/golden/make_png_golden.py
"""
import os
import struct
import zlib

import numpy as np

BLOCK = 4096
# RFC 1951 3.2.5: symbol 257 + k has base length LENGTH_BASE[k] and LENGTH_EXTRA[k] extra bits
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
PALETTE = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0)]


class Bits:
    def __init__(self):
        self.bits = []

    def value(self, v, n):                      # n bits of v, least significant first (headers, extra bits)
        self.bits.extend((v >> k) & 1 for k in range(n))

    def huffman(self, code, n):                 # a Huffman code: most significant bit first
        self.bits.extend((code >> k) & 1 for k in range(n - 1, -1, -1))

    def symbol(self, s):                        # RFC 1951 3.2.6, the fixed literal / length code
        if s < 144:
            self.huffman(0b00110000 + s, 8)
        elif s < 256:
            self.huffman(0b110010000 + s - 144, 9)
        elif s < 280:
            self.huffman(s - 256, 7)
        else:
            self.huffman(0b11000000 + s - 280, 8)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def deflate(raw):
    out = Bits()
    n = len(raw)
    for b0 in range(0, n, BLOCK):
        b1 = min(b0 + BLOCK, n)
        out.value(1 if b1 == n else 0, 1)
        out.value(1, 2)
        p = b0
        while p < b1:
            run = 0
            while p > 0 and run < min(258, b1 - p) and raw[p + run] == raw[p + run - 1]:
                run += 1
            if run >= 3:
                k = max(i for i in range(29) if LENGTH_BASE[i] <= run and (i < 28 or run == 258))
                out.symbol(257 + k)
                out.value(run - LENGTH_BASE[k], LENGTH_EXTRA[k])
                out.huffman(0, 5)               # distance 1: code 0, no extra bits
                p += run
            else:
                out.symbol(raw[p])
                p += 1
        out.symbol(256)
    return out.bytes()


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png(pixels, rows):
    h, w = pixels.shape
    if pixels.dtype == np.uint8:
        samples, colour = pixels, 0
    else:
        v = pixels.astype(np.int64)
        samples, colour = np.where((v >= -1) & (v < rows), v + 1, 0).astype(np.uint8), 3
    raw = np.concatenate([np.zeros((h, 1), np.uint8), samples], axis=1).tobytes()
    stream = b"\x78\x01" + deflate(raw) + struct.pack(">I", zlib.adler32(raw))
    assert zlib.decompress(stream) == raw
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0))
    if colour == 3:
        out += chunk(b"PLTE", bytes(3) + b"".join(bytes(PALETTE[(k - 1) % 4]) for k in range(1, rows + 1))) + chunk(b"tRNS", b"\0")
    return out + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def blobs(rng, h, w, ids, background):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.full((h, w), background, np.int64)
    for i in ids:
        cy, cx, ry, rx = rng.integers(0, h), rng.integers(0, w), rng.integers(2, max(3, h // 5)), rng.integers(2, max(3, w // 5))
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = i
    return m


def cases():
    rng = np.random.default_rng(20240607)
    c = {}
    c["one_pixel"] = (np.array([[7]], np.uint8), 0)
    c["one_block"] = (blobs(rng, 1, 4095, [40, 80, 200, 120, 160, 250, 9, 33], 0).astype(np.uint8), 0)       # N = 4096: exactly one block
    c["second_block"] = (blobs(rng, 1, 4096, [40, 80, 200, 120, 160, 250, 9, 33], 0).astype(np.uint8), 0)    # N = 4097: a second block of one byte
    c["zeros_2x4095"] = (np.zeros((2, 4095), np.uint8), 0)                                                    # the second block starts inside a run
    c["three_rows"] = (blobs(rng, 3, 2047, [1, 2, 3, 255, 144, 143], 0).astype(np.uint8), 0)                 # N = 6144
    lengths = [1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519]
    values = [10, 200, 30, 220, 50, 240, 70, 150, 90, 143, 144, 255]                                          # neighbours differ, the first is not the filter byte's 0
    c["runs"] = (np.concatenate([np.full(n, v, np.uint8) for n, v in zip(lengths, values)])[None, :], 0)
    c["random"] = (rng.integers(0, 256, (70, 61), dtype=np.uint8), 0)
    m = blobs(rng, 120, 200, list(rng.permutation(255)[:40]) + [254, 0], -1)
    m[5, 7], m[100, 150] = 300, -2
    c["instance_255"] = (m.astype(np.int16), 255)
    m = blobs(rng, 33, 47, [0, 0, 0], -1)
    m[3, 3], m[30, 40] = 1, -2                                                                                # outside -1 .. rows - 1: index 0
    c["instance_1"] = (m.astype(np.int16), 1)
    return c


def main():
    out = {}
    for name, (pixels, rows) in cases().items():
        out[name + "_pixels"] = pixels
        out[name + "_rows"] = np.int32(rows)
        out[name + "_file"] = np.frombuffer(png(pixels, rows), dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {n[:-5]: int(v.size) for n, v in out.items() if n.endswith("_file")})


if __name__ == "__main__":
    main()
