"""JPEG files in: the mirror of the ``mrcnn_jpeg_*`` entries of include/maskrcnn_hip.h.

Baseline JPEG (grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0) decoded to libjpeg's bytes: the entropy decoder on the host, dequantisation,
inverse DCT, chroma upsampling and colour conversion on the GPU.  ``info`` and ``decode_host`` need no GPU; ``decode_host`` is the
scalar definition ``decode_batch`` is held to.

JPEG files out: ``encode_host`` is the scalar definition of the encoder (libjpeg's default compressor: Annex K tables at a quality,
the standard Huffman tables), ``encode_batch`` the same files from the GPU, where every stage of the encoder runs; only the files'
bytes come back.  No codec is imported here."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, _marshal


def _view(data) -> np.ndarray:
    a = np.frombuffer(data, dtype=np.uint8)
    if a.size == 0:
        raise ValueError("an empty JPEG file")
    return a


def file_table(files: Sequence[bytes]):
    """list of bytes-like → (mrcnn_jpeg table, the arrays that keep the bytes alive)."""
    keep = [_view(f) for f in files]
    table = (_lib.Jpeg * max(1, len(keep)))()
    for b, a in enumerate(keep):
        table[b].data, table[b].length = a.ctypes.data, a.size
    return table, keep


def info(data) -> dict:
    """{"height", "width", "components", "h_samp", "v_samp"} of a JPEG file (``mrcnn_jpeg_info``); raises MrcnnError for a file
    outside the decoder's scope (code 5, the message names what was found) or a damaged one (code 2)."""
    a = _view(data)
    v = [C.c_int32(0) for _ in range(5)]
    _lib.check(_lib.lib().mrcnn_jpeg_info(a.ctypes.data, a.size, *[C.byref(x) for x in v]))
    return dict(zip(("height", "width", "components", "h_samp", "v_samp"), (int(x.value) for x in v)))


def decode_host(data) -> np.ndarray:
    """(h, w, 3) uint8 RGB of a JPEG file, the whole pipeline on the host (``mrcnn_jpeg_decode_host``)."""
    a = _view(data)
    i = info(a)
    rgb = np.empty((i["height"], i["width"], 3), dtype=np.uint8)
    _lib.check(_lib.lib().mrcnn_jpeg_decode_host(a.ctypes.data, a.size, rgb.ctypes.data, rgb.size))
    return rgb


ENTROPY = {"host": 0, "device": 1}


def entropy_code(entropy) -> int:
    """"host" | "device" → MRCNN_JPEG_ENTROPY_*; an integer goes through as it is (the library refuses what it does not know)."""
    if isinstance(entropy, str):
        if entropy not in ENTROPY:
            raise ValueError(f"entropy {entropy!r}: expected one of {sorted(ENTROPY)}")
        return ENTROPY[entropy]
    return int(entropy)


def decode_batch(files: Sequence[bytes], device: bool = True, entropy="host") -> Tuple[list, List[Tuple[int, int]]]:
    """A batch of JPEG files of any sizes in one call (``mrcnn_jpeg_decode_batch_on``) → ([ (h_b, w_b, 3) uint8 ], [(h_b, w_b)]).
    device=True: CUDA tensors, views of one allocation (the decoded images never exist in host memory); False: numpy arrays.
    entropy: "host" (the default) decodes the Huffman streams on the host; "device" (opt-in) on the GPU — self-synchronising parallel
    decoding: the files' bytes go up instead of their coefficients, and a file the device's verdict does not call clean is decoded by
    the host after all, so the bytes, and the error for a damaged file, are the same either way."""
    files = list(files)
    B = len(files)
    entropy = entropy_code(entropy)
    sizes = []
    for f in files:
        i = info(f)
        sizes.append((i["height"], i["width"]))
    offsets = np.zeros(max(1, B), dtype=np.int64)
    total = 0
    for b, (h, w) in enumerate(sizes):
        offsets[b] = total
        total += (h * w * 3 + 15) // 16 * 16
    table, keep = file_table(files)
    hs, ws = np.zeros(max(1, B), np.int32), np.zeros(max(1, B), np.int32)
    if device:
        import torch
        buf = torch.empty(max(total, 16), dtype=torch.uint8, device="cuda")
        ptr, space = buf.data_ptr(), _lib.DEVICE
    else:
        buf = np.empty(max(total, 16), dtype=np.uint8)
        ptr, space = buf.ctypes.data, _lib.HOST
    _lib.check(_lib.lib().mrcnn_jpeg_decode_batch_on(table, B, space, entropy, ptr, offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data))
    del keep
    got = [(int(hs[b]), int(ws[b])) for b in range(B)]
    images = [buf[int(offsets[b]):int(offsets[b]) + h * w * 3].reshape(h, w, 3) for b, (h, w) in enumerate(got)]
    return images, got


def coefficients(files: Sequence[bytes], entropy=0, unit_bytes: int = 0, max_rounds: int = 0):
    """Test entry ``mrcnn_jpeg_coefficients`` (include/maskrcnn_hip_test.h): the quantised coefficients of a batch from the host decoder
    (entropy 0), the device entropy stage (1) or its sequential host model (2) → (coef int16 (blocks, 64), block0 int64 (B + 1),
    stats = [clean, fell back, rounds, units]).  unit_bytes / max_rounds: its knobs (0 = production)."""
    files = list(files)
    B = len(files)
    table, keep = file_table(files)
    block0 = np.zeros(B + 1, np.int64)
    stats = np.zeros(4, np.int32)
    e = entropy_code(entropy)
    code = _lib.lib().mrcnn_jpeg_coefficients(table, B, e, int(unit_bytes), int(max_rounds), None, 0, block0.ctypes.data, stats.ctypes.data)
    if code != 4 or int(block0[B]) <= 0:            # MRCNN_ERR_SHAPE from the capacity check is the sizing answer
        _lib.check(code)
    coef = np.zeros((int(block0[B]), 64), np.int16)
    _lib.check(_lib.lib().mrcnn_jpeg_coefficients(table, B, e, int(unit_bytes), int(max_rounds), coef.ctypes.data, coef.size, block0.ctypes.data,
                                                  stats.ctypes.data))
    del keep
    return coef, block0, stats


SAMPLING = {"444": 0, "422": 1, "420": 2, "grey": 3, "gray": 3}


def _sampling(sampling) -> int:
    if isinstance(sampling, str):
        if sampling not in SAMPLING:
            raise ValueError(f"sampling {sampling!r}: expected one of {sorted(SAMPLING)}")
        return SAMPLING[sampling]
    return int(sampling)


def encode_host(rgb, quality: int = 90, sampling="420") -> bytes:
    """An (h, w, 3) uint8 RGB image → the bytes of a baseline JPEG file, the whole encoder on the host (``mrcnn_jpeg_encode_host``):
    the definition ``encode_batch`` is held to.  sampling: "444", "422", "420" or "grey" (one component, the luma)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"the image has shape {tuple(rgb.shape)}, expected (h, w, 3)")
    h, w, s = int(rgb.shape[0]), int(rgb.shape[1]), _sampling(sampling)
    n = C.c_int64(0)
    _lib.check(_lib.lib().mrcnn_jpeg_encode_host(rgb.ctypes.data, h, w, int(quality), s, None, 0, C.byref(n)))
    out = np.empty(int(n.value), dtype=np.uint8)
    _lib.check(_lib.lib().mrcnn_jpeg_encode_host(rgb.ctypes.data, h, w, int(quality), s, out.ctypes.data, out.size, C.byref(n)))
    return out.tobytes()


def image_table(images):
    """list of (h, w, 3) uint8 numpy arrays or CUDA tensors → (mrcnn_image table, memspace, what keeps the pixels alive)."""
    table, space, keep, _, _ = _marshal.image_table(images)
    return table, space.code, keep


def encode_batch(images, quality: int = 90, sampling="420") -> List[bytes]:
    """A batch of images of any sizes → their JPEG files in one call (``mrcnn_jpeg_encode_batch``), byte for byte what
    ``encode_host`` writes for each.  images: numpy arrays (copied up) or uint8 CUDA tensors (read in place, e.g. what
    ``detection.render_detections_source`` left on the device).  The buffer is sized from the call's own answer: a first attempt
    at one byte per pixel, and when that is too small, a second at the size the first one reported."""
    table, space, keep = image_table(images)
    B = len(keep)
    if B == 0:
        return []
    offsets = np.zeros(B + 1, dtype=np.int64)
    capacity = max(4096, sum(int(im.shape[0]) * int(im.shape[1]) for im in keep) + 1024 * B)
    for _ in range(2):
        out = np.empty(capacity, dtype=np.uint8)
        code = _lib.lib().mrcnn_jpeg_encode_batch(table, B, space, int(quality), _sampling(sampling), out.ctypes.data, out.size, offsets.ctypes.data)
        if code == 4 and int(offsets[B]) > capacity:        # MRCNN_ERR_SHAPE from the capacity check: offsets[B] is the size needed
            capacity = int(offsets[B])
            continue
        _lib.check(code)
        break
    else:
        _lib.check(code)
    del keep
    return [out[int(offsets[b]):int(offsets[b + 1])].tobytes() for b in range(B)]
