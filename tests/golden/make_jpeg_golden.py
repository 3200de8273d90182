"""Writes tests/golden/jpeg_v1.npz: small synthetic JPEG files (PIL / libjpeg-turbo encodes them) and the RGB that PIL decodes from
each — libjpeg's default pipeline (JDCT_ISLOW, fancy upsampling), which DEFINES the output of mrcnn_jpeg_decode_host and
mrcnn_jpeg_decode_batch.  The only place that imports PIL; the tests read the .npz.

    python tests/golden/make_jpeg_golden.py

Per case NAME the file holds NAME_jpg (the file's bytes, uint8), NAME_rgb ((h, w, 3) uint8, absent for the refused case) and
NAME_info = [height, width, components, h_samp, v_samp].  Images are gradients plus seeded noise, so the AC coefficients are dense."""
import io
import os

import numpy as np
from PIL import Image

# name: (height, width, mode, save options)      subsampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0
CASES = [
    ("one_pixel", 1, 1, "RGB", dict(quality=75, subsampling=2)),
    ("one_block", 8, 8, "RGB", dict(quality=75, subsampling=0)),
    ("one_over", 9, 9, "RGB", dict(quality=75, subsampling=0)),
    ("exact_mcu", 16, 16, "RGB", dict(quality=75, subsampling=2)),
    ("odd_444", 17, 23, "RGB", dict(quality=90, subsampling=0)),
    ("odd_422", 33, 47, "RGB", dict(quality=75, subsampling=1)),
    ("odd_420", 35, 45, "RGB", dict(quality=75, subsampling=2)),
    ("narrow", 31, 9, "RGB", dict(quality=100, subsampling=2)),
    ("custom_tables", 64, 64, "RGB", dict(quality=50, subsampling=2, optimize=True)),
    ("restarts", 70, 90, "RGB", dict(quality=80, subsampling=2, restart_marker_blocks=3)),
    ("coarse", 40, 40, "RGB", dict(quality=3, subsampling=2)),
    ("grey", 40, 40, "L", dict(quality=75)),
    ("saturated", 24, 24, "RGB", dict(quality=100, subsampling=0)),
    ("refused", 40, 40, "RGB", dict(quality=75, subsampling=2, progressive=True)),
]
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


def synthetic(name, h, w, mode, rng):
    if name == "saturated":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)          # uniform noise over 0..255: every clamp
    yy, xx = np.mgrid[0:h, 0:w]
    planes = [(xx * 7 + yy * 3) % 256, (yy * 5 + xx * 2 + 40) % 256, ((xx + yy) * 4 + 90) % 256]
    img = np.stack(planes, -1).astype(np.int32) + rng.integers(-48, 49, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., 0] if mode == "L" else img


def markers(data):
    """The second bytes of the file's markers up to SOS."""
    out, pos = [], 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        out.append(m)
        if m == 0xDA:
            break
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    return out


def main():
    rng = np.random.default_rng(20260101)
    out = {}
    for name, h, w, mode, opts in CASES:
        img = synthetic(name, h, w, mode, rng)
        bio = io.BytesIO()
        Image.fromarray(img, mode).save(bio, "JPEG", **opts)
        data = bio.getvalue()
        ms = markers(data)
        assert (0xC2 in ms) == (name == "refused"), (name, ms)
        assert (0xDD in ms) == (name == "restarts"), (name, ms)
        comps = 1 if mode == "L" else 3
        hs, vs = (1, 1) if mode == "L" else SAMPLING[opts["subsampling"]]
        out[name + "_jpg"] = np.frombuffer(data, np.uint8)
        out[name + "_info"] = np.array([h, w, comps, hs, vs], np.int32)
        if name != "refused":
            out[name + "_rgb"] = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", sum(v.size for k, v in out.items() if k.endswith("_jpg")), "bytes of JPEG")


if __name__ == "__main__":
    main()
