"""JPEG files in: the mirror of the ``mrcnn_jpeg_*`` entries of include/maskrcnn_hip.h.

Baseline JPEG (grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0) decoded to libjpeg's bytes: the entropy decoder on the host, dequantisation,
inverse DCT, chroma upsampling and colour conversion on the GPU.  ``info`` and ``decode_host`` need no GPU; ``decode_host`` is the
scalar definition ``decode_batch`` is held to.  No codec is imported here."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib


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


def decode_batch(files: Sequence[bytes], device: bool = True) -> Tuple[list, List[Tuple[int, int]]]:
    """A batch of JPEG files of any sizes in one call (``mrcnn_jpeg_decode_batch``) → ([ (h_b, w_b, 3) uint8 ], [(h_b, w_b)]).
    device=True: CUDA tensors, views of one allocation (the decoded images never exist in host memory); False: numpy arrays."""
    files = list(files)
    B = len(files)
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
    _lib.check(_lib.lib().mrcnn_jpeg_decode_batch(table, B, space, ptr, offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data))
    del keep
    got = [(int(hs[b]), int(ws[b])) for b in range(B)]
    images = [buf[int(offsets[b]):int(offsets[b]) + h * w * 3].reshape(h, w, 3) for b, (h, w) in enumerate(got)]
    return images, got
