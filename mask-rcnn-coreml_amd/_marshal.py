"""What the bindings of the image-space entries share (detection.py, models.py, jpeg.py): the switch between numpy arrays and CUDA
tensors, the ``mrcnn_image`` table, sizes as arrays, the 16-byte layout of a ragged output and the capacity retry of the entries
that return run lengths.  Private: the public functions keep their own argument checks and docstrings."""
from __future__ import annotations

import numpy as np

from . import _lib


class Space:
    """Where the arrays of one call live: numpy arrays (MRCNN_HOST) or CUDA tensors of one device (MRCNN_DEVICE)."""

    def __init__(self, like=None):
        """like: an array of the call (numpy or CUDA tensor), a torch device, or None for the host"""
        self.device = None if like is None or isinstance(like, np.ndarray) else getattr(like, "device", like)
        self.on_host = self.device is None
        self.code = _lib.HOST if self.on_host else _lib.DEVICE
        self.ptr = (lambda a: a.ctypes.data) if self.on_host else (lambda a: a.data_ptr())      # the address of an array of this space

    def new(self, shape, dtype, zero=False):
        """An array of this space; uint32 is int32 on the device (torch has no uint32 tensors to compute with)."""
        if self.on_host:
            return (np.zeros if zero else np.empty)(shape, dtype)
        import torch
        dt = getattr(torch, np.dtype(dtype).name.replace("uint32", "int32"))
        return (torch.zeros if zero else torch.empty)(shape, dtype=dt, device=self.device)

    def f32(self, *arrays):
        """The arrays as contiguous float32 of this space: numpy arrays converted, CUDA tensors checked and used in place."""
        if self.on_host:
            return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        import torch
        assert all(a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() for a in arrays)
        return list(arrays)


def sizes_of(sizes):
    """[(h_b, w_b)] → (hs, ws), int32 arrays"""
    return np.array([int(s[0]) for s in sizes], dtype=np.int32), np.array([int(s[1]) for s in sizes], dtype=np.int32)


def image_table(images, space=None):
    """A list of (h, w, 3) uint8 images, numpy arrays or CUDA tensors (space = None: as the first one says) → (mrcnn_image table,
    Space, what keeps the pixels alive, hs, ws)."""
    images = list(images)
    space = space or Space(images[0] if images else None)
    table = (_lib.Image * max(1, len(images)))()
    keep, hs, ws = [], [], []
    for b, im in enumerate(images):
        if space.on_host:
            im = np.ascontiguousarray(im, dtype=np.uint8)
        else:
            import torch
            if not (im.is_cuda and im.dtype == torch.uint8):
                raise ValueError(f"image {b}: expected a uint8 CUDA tensor")
            im = im.contiguous()
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"image {b} has shape {tuple(im.shape)}, expected (h, w, 3)")
        keep.append(im), hs.append(int(im.shape[0])), ws.append(int(im.shape[1]))
        table[b].rgb, table[b].height, table[b].width = space.ptr(im), hs[b], ws[b]
    return table, space, keep, np.array(hs, dtype=np.int32), np.array(ws, dtype=np.int32)


def ragged_output(space, hs, ws, dtype, lead=(), trail=()):
    """One buffer for a ragged batch: image b is a (*lead, h_b, w_b, *trail) array of ``dtype`` that starts on a 16-byte boundary.
    Returns (buffer, the byte offsets as int64, views): views() gives the per-image arrays once the library has written them."""
    item, per_pixel, hw = np.dtype(dtype).itemsize, 1, list(zip(hs.tolist(), ws.tolist()))
    for d in lead + trail:
        per_pixel *= int(d)
    starts, at = [], 0                                       # (plain ints: a batch is a few images, and the call is timed with its binding)
    for h, w in hw:
        starts.append(at)
        at += (max(1, per_pixel) * h * w * item + 15) // 16 * 16
    out = space.new(max(1, at // item), dtype)

    def views():
        return [out[s // item:s // item + per_pixel * h * w].reshape(*lead, h, w, *trail) for s, (h, w) in zip(starts, hw)]
    return out, np.array(starts, dtype=np.int64), views


def rle_results(space, B, per, hs, ws, capacity, call, resident=None):
    """The run lengths of B images x ``per`` RLEs: call(counts, capacity, run_offsets) -> status runs with a first guess of the
    capacity and, if the library answers MRCNN_ERR_SHAPE with the offsets complete (the capacity was the reason), once more with
    the need it reported.  Returns rles[b][i] = {"size": [h_b, w_b], "counts": uint32 runs}; only the used runs cross to the host.
    resident: a list that receives the (counts, run_offsets) pair as the library wrote it, in the call's own memory space."""
    n = max(0, B * per)
    offs_buf = space.new(n + 1, np.int64, zero=True)
    for _ in range(2):
        counts = space.new(max(1, capacity), np.uint32)
        st = call(counts, capacity, offs_buf)
        offsets = offs_buf if space.on_host else offs_buf.cpu().numpy()
        if st != 4 or int(offsets[n]) <= capacity:
            break
        capacity = int(offsets[n])
    _lib.check(st)
    used = int(offsets[n])
    if resident is not None:
        resident.append((counts[:used], offs_buf))
    host = counts[:used] if space.on_host else counts[:used].cpu().numpy().view(np.uint32)
    return [[{"size": [int(hs[b]), int(ws[b])], "counts": host[int(offsets[b * per + i]):int(offsets[b * per + i + 1])]}
             for i in range(per)] for b in range(B)]
