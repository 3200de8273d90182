"""The synthetic images of make_jpeg_entropy_golden.py (numpy only): the tests rebuild the larger file's image from its seed."""
import numpy as np


def synthetic(h, w, mode, rng, noise=48):
    yy, xx = np.mgrid[0:h, 0:w]
    planes = [(xx * 7 + yy * 3) % 256, (yy * 5 + xx * 2 + 40) % 256, ((xx + yy) * 4 + 90) % 256]
    img = np.stack(planes, -1).astype(np.int32) + rng.integers(-noise, noise + 1, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., 0] if mode == "L" else img


def large_image(seed):
    """The 240x320 noise-on-gradient image of the larger file."""
    return synthetic(240, 320, "RGB", np.random.default_rng(seed))
