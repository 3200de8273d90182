"""What tests/test_jpeg_entropy_host.py and tests/test_gpu_jpeg_entropy.py share: the files (jpeg_v1.npz's decodable cases,
jpeg_entropy_v1.npz, and the one larger file generated here), the damaged variants of a file, and the calls into
mrcnn_jpeg_coefficients.  Not a test module."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD1 = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_v1.npz"))
GOLD2 = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_entropy_v1.npz"))
HOST, DEVICE, MODEL = 0, 1, 2
PRODUCTION_UNIT = 128


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def _large():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        maker = importlib.import_module("make_jpeg_entropy_golden_images")
    finally:
        sys.path.pop(0)
    return _mod("jpeg").encode_host(maker.large_image(int(GOLD2["large_seed"][0])), 90, "420")


_FILES = None


def files():
    """{name: bytes}, built once: 25 files — jpeg_v1.npz's 13 decodable ones, jpeg_entropy_v1.npz's 11 (as entropy_NAME) and `large` (240x320 4:2:0 q90 through jpeg.encode_host, about 56 KB)."""
    global _FILES
    if _FILES is None:
        f = {k[:-4]: GOLD1[k].tobytes() for k in GOLD1.files if k.endswith("_jpg") and k[:-4] + "_rgb" in GOLD1.files}
        f.update({"entropy_" + k[:-4]: GOLD2[k].tobytes() for k in GOLD2.files if k.endswith("_jpg")})
        f["large"] = _large()
        _FILES = f
    return _FILES


def scan_start(data):
    pos = 2
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        pos += 2 + n
        if m == 0xDA:
            return pos


def stuffed_at_unit_end(data, unit):
    """Stuffed FF 00 pairs of the scan whose FF is the last byte of a `unit`-byte unit counted from the scan's first byte."""
    a = np.frombuffer(data, np.uint8)
    s = scan_start(data)
    ff = np.flatnonzero((a[s:-1] == 0xFF) & (a[s + 1:] == 0x00))
    return int((ff % unit == unit - 1).sum())


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


def damaged(data, seed):
    """[(label, bytes)]: the five truncations and 20 seeded single-byte corruptions inside the scan."""
    s, n = scan_start(data), len(data)
    rst = [i for i in range(s, n - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    cuts = [("header", s // 2), ("first scan byte", s + 1), ("mid-scan", (s + n) // 2), ("before a marker", rst[0] if rst else n - 2), ("no EOI", n - 1)]
    out = [("cut " + label, data[:k]) for label, k in cuts]
    rng = np.random.default_rng(seed)
    for i in range(20):
        at, flip = int(rng.integers(s, n - 2)), int(rng.integers(1, 256))
        b = bytearray(data)
        b[at] ^= flip
        out.append((f"flip {i} (byte {at} ^ {flip:02x})", bytes(b)))
    return out


def coefficients(batch, entropy, unit_bytes=0, max_rounds=0):
    """mrcnn_jpeg_coefficients → (status, message, coef or None, stats)."""
    L, J = _mod("_lib"), _mod("jpeg")
    table, keep = J.file_table(batch)
    B = len(batch)
    block0, stats = np.zeros(B + 1, np.int64), np.zeros(4, np.int32)
    st = L.lib().mrcnn_jpeg_coefficients(table, B, entropy, unit_bytes, max_rounds, None, 0, block0.ctypes.data, stats.ctypes.data)
    if st != 4 or block0[B] <= 0:
        return st, L.lib().mrcnn_last_error().decode(), None, stats
    coef = np.zeros((int(block0[B]), 64), np.int16)
    st = L.lib().mrcnn_jpeg_coefficients(table, B, entropy, unit_bytes, max_rounds, coef.ctypes.data, coef.size, block0.ctypes.data, stats.ctypes.data)
    del keep
    return st, (L.lib().mrcnn_last_error().decode() if st else ""), (coef if st == 0 else None), stats


_HOST = {}


def host_coefficients(names):
    """The host decoder's coefficients of a batch of intact files, computed once per batch and shared."""
    key = tuple(names)
    if key not in _HOST:
        st, msg, coef, _ = coefficients([files()[n] for n in names], HOST)
        assert st == 0, msg
        coef.setflags(write=False)
        _HOST[key] = coef
    return _HOST[key]
