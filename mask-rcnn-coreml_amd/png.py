"""PNG files out: the mirror of the ``mrcnn_png_*`` entries of include/maskrcnn_hip.h.

Label images leave as lossless files: a uint8 plane (a mask of ``detection.paste_masks_source``, a class map) as 8-bit greyscale, an
int16 instance map (``detection.instance_map_source``) as an 8-bit palette image whose index is id + 1, coloured like the rendered
overlays, with "no detection" transparent.  ``encode_host`` is the sequential definition and needs no GPU; ``encode_batch`` returns
the same files from the GPU, where the deflate stream is made — only the files' bytes come back.  ``parse`` reads such a file back
with ``zlib`` and ``struct`` alone.  No codec is imported to write."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import List

import numpy as np

from . import _lib

GREY8, INSTANCE = 0, 1
BLOCK_BYTES = 4096


def _format(dtype, rows, what="the image"):
    """numpy dtype → (MRCNN_PNG_*, rows as the library takes it)."""
    if dtype == np.uint8:
        return GREY8, 0 if rows is None else int(rows)
    if dtype == np.int16:
        if rows is None:
            raise ValueError(f"{what} is an int16 instance map: rows (the number of detection rows, 1..255) is required")
        return INSTANCE, int(rows)
    raise ValueError(f"{what} has dtype {dtype}: expected uint8 (a plane, written as greyscale) or int16 (an instance map)")


def encode_host(pixels, rows=None) -> bytes:
    """An (h, w) uint8 plane or int16 instance map → the bytes of a PNG file, the whole encoder on the host
    (``mrcnn_png_encode_host``): the definition ``encode_batch`` is held to.  rows: required for an int16 map, the number of
    detection rows (values -1 .. rows - 1 are written as index v + 1, anything else as 0)."""
    pixels = np.ascontiguousarray(pixels)
    if pixels.ndim != 2:
        raise ValueError(f"the image has shape {tuple(pixels.shape)}, expected (h, w)")
    fmt, rows = _format(pixels.dtype, rows)
    h, w = int(pixels.shape[0]), int(pixels.shape[1])
    n = C.c_int64(0)
    _lib.check(_lib.lib().mrcnn_png_encode_host(pixels.ctypes.data, h, w, fmt, rows, None, 0, C.byref(n)))
    out = np.empty(int(n.value), dtype=np.uint8)
    _lib.check(_lib.lib().mrcnn_png_encode_host(pixels.ctypes.data, h, w, fmt, rows, out.ctypes.data, out.size, C.byref(n)))
    return out.tobytes()


def source_table(images):
    """list of (h, w) numpy arrays or CUDA tensors, all uint8 or all int16 → (mrcnn_png_source table, memspace, numpy dtype, what
    keeps the pixels alive)."""
    images = list(images)
    table = (_lib.PngSource * max(1, len(images)))()
    on_host = len(images) == 0 or isinstance(images[0], np.ndarray)
    keep, dtype = [], None
    for b, im in enumerate(images):
        if on_host:
            im = np.ascontiguousarray(im)
            ptr, dt = im.ctypes.data, im.dtype
        else:
            import torch
            if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype in (torch.uint8, torch.int16)):
                raise ValueError(f"image {b}: expected a uint8 or int16 CUDA tensor")
            im = im.contiguous()
            ptr, dt = im.data_ptr(), np.dtype(np.uint8 if im.dtype == torch.uint8 else np.int16)
        if im.ndim != 2:
            raise ValueError(f"image {b} has shape {tuple(im.shape)}, expected (h, w)")
        if dtype is not None and dt != dtype:
            raise ValueError(f"image {b} has dtype {dt}, image 0 has {dtype}: a call writes one format")
        dtype = dt
        keep.append(im)
        table[b].pixels, table[b].height, table[b].width = ptr, int(im.shape[0]), int(im.shape[1])
    return table, (_lib.HOST if on_host else _lib.DEVICE), dtype, keep


def encode_batch(images, rows=None) -> List[bytes]:
    """A batch of planes or maps of any sizes → their PNG files in one call (``mrcnn_png_encode_batch``), byte for byte what
    ``encode_host`` writes for each.  images: numpy arrays (copied up) or CUDA tensors (read in place, e.g. what
    ``detection.instance_map_source`` left on the device); uint8 2-D → greyscale, int16 2-D → instance files, for which ``rows`` is
    required.  The buffer is sized from the call's own answer: a first attempt at a quarter byte per pixel, and when that is too
    small, a second at the size the first one reported."""
    table, space, dtype, keep = source_table(images)
    B = len(keep)
    if B == 0:
        return []
    fmt, rows = _format(dtype, rows, "the batch")
    offsets = np.zeros(B + 1, dtype=np.int64)
    capacity = max(4096, sum(int(im.shape[0]) * int(im.shape[1]) for im in keep) // 4 + 1024 * B)
    for _ in range(2):
        out = np.empty(capacity, dtype=np.uint8)
        code = _lib.lib().mrcnn_png_encode_batch(table, B, space, fmt, rows, out.ctypes.data, out.size, offsets.ctypes.data)
        if code == 4 and int(offsets[B]) > capacity:        # MRCNN_ERR_SHAPE from the capacity check: offsets[B] is the size needed
            capacity = int(offsets[B])
            continue
        _lib.check(code)
        break
    else:
        _lib.check(code)
    del keep
    return [out[int(offsets[b]):int(offsets[b + 1])].tobytes() for b in range(B)]


def parse(data) -> dict:
    """A PNG file as this module writes them, read back with ``zlib`` and ``struct`` only → {"chunks": [(type, data, crc_ok)],
    "width", "height", "bit_depth", "colour_type", "compression", "filter", "interlace", "palette": (n, 3) uint8 or None,
    "transparency": bytes or None, "scanlines": (h, w) uint8 — the samples (for a palette file the indices: id = index - 1),
    "filters": (h,) uint8}.  Raises ValueError for anything that is not an 8-bit greyscale or palette file without interlacing
    and with filter 0 on every row."""
    data = bytes(data)
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file: the signature is missing")
    chunks, at = [], 8
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError(f"a truncated chunk at byte {at}")
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if at + 12 + n > len(data):
            raise ValueError(f"chunk {kind!r} at byte {at} runs over the end of the file")
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        chunks.append((kind.decode("latin-1"), body, zlib.crc32(kind + body) == crc))
        at += 12 + n
    if not chunks or chunks[0][0] != "IHDR" or len(chunks[0][1]) != 13 or chunks[-1][0] != "IEND":
        raise ValueError("IHDR must come first and IEND last")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or colour not in (0, 3) or comp != 0 or filt != 0 or lace != 0:
        raise ValueError(f"depth {depth}, colour type {colour}, interlace {lace}: only 8-bit greyscale / palette files without interlacing are read")
    find = lambda kind: [c[1] for c in chunks if c[0] == kind]
    raw = np.frombuffer(zlib.decompress(b"".join(find("IDAT"))), dtype=np.uint8)
    if raw.size != h * (w + 1):
        raise ValueError(f"IDAT inflates to {raw.size} bytes, a {h}x{w} image has {h * (w + 1)}")
    lines = raw.reshape(h, w + 1)
    if lines[:, 0].any():
        raise ValueError("a row filter other than 0")
    plte, trns = find("PLTE"), find("tRNS")
    return {"chunks": chunks, "width": w, "height": h, "bit_depth": depth, "colour_type": colour, "compression": comp, "filter": filt,
            "interlace": lace, "palette": np.frombuffer(plte[0], dtype=np.uint8).reshape(-1, 3) if plte else None,
            "transparency": trns[0] if trns else None, "scanlines": lines[:, 1:].copy(), "filters": lines[:, 0].copy()}
