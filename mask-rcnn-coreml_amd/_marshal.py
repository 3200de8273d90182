"""What the bindings of the image-space entries share (detection.py, models.py, jpeg.py): the switch between numpy arrays and CUDA
tensors, the ``mrcnn_image`` table, sizes as arrays, the 16-byte layout of a ragged output, the RLE set of a call and the capacity
retry of the entries that return run lengths.  Private: the public functions keep their own argument checks and docstrings."""
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

    def host(self, a):
        """An array of this space as a numpy array: as it is, or read back."""
        return a if self.on_host else a.cpu().numpy()

    def take(self, a, dtype):
        """Any array (numpy or tensor; None stays None) as a contiguous array of this space: converted or moved only where it has to be."""
        if a is None:
            return None
        if self.on_host:
            return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "is_cuda") else a, dtype=dtype)
        import torch
        t = a if hasattr(a, "is_cuda") else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
        return t.to(device=self.device, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()


HOST = Space()


def choice(table, value, message):
    """A name of ``table`` or one of its codes → the code; anything else is a ValueError with ``message``."""
    if value not in table and value not in table.values():
        raise ValueError(message)
    return table.get(value, value)


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


def addressable(counts):
    """Run lengths the library can be handed: empty numpy counts become one zero word (an empty array has no address worth passing)."""
    return np.zeros(1, np.uint32) if isinstance(counts, np.ndarray) and counts.size == 0 else counts


def rle_set(name, rles, sizes, device):
    """An RLE set for the library: (counts, run_offsets, B, slots, hs, ws).  ``rles`` is either what merge_tiles, unite_tiles and
    masks_rle_source return — rles[b][i] = {"size": [h_b, w_b], "counts": uint32 runs}, the same number of slots for every image —
    or a (counts, run_offsets) pair holding B*slots RLEs, numpy arrays or CUDA tensors, which then needs ``sizes`` = [(h_b, w_b)].
    device = None: numpy arrays (a pair of tensors is copied to the host); else CUDA tensors on that device — a pair of CUDA tensors
    is used in place, anything else is uploaded (a few MB)."""
    if is_pair(rles):
        counts, offs = rles
        if sizes is None:
            raise ValueError(f"{name}: a (counts, run_offsets) pair needs sizes = [(h_b, w_b)]")
        B = len(sizes)
        n = int(offs.shape[0]) - 1
        slots = n // B if B else 0
        if n != B * slots or n < 0:
            raise ValueError(f"{name}: run_offsets holds {n} RLEs, not a multiple of the {B} images")
        if not isinstance(counts, np.ndarray):
            import torch
            assert counts.is_cuda and offs.is_cuda and counts.element_size() == 4 and offs.dtype == torch.int64 and counts.is_contiguous() and offs.is_contiguous()
            if device is None:
                counts, offs = counts.cpu().numpy().view(np.uint32), offs.cpu().numpy()
        else:
            counts, offs = np.ascontiguousarray(counts, dtype=np.uint32), np.ascontiguousarray(offs, dtype=np.int64)
    else:
        rows = [list(r) for r in rles]
        B = len(rows)
        slots = len(rows[0]) if B else 0
        if any(len(r) != slots for r in rows):
            raise ValueError(f"{name}: every image needs the same number of RLEs (pad with empty masks)")
        if sizes is None:
            if B and not slots:
                raise ValueError(f"{name}: images without RLEs need sizes = [(h_b, w_b)]")
            sizes = [r[0]["size"] for r in rows]
        if len(sizes) != B:
            raise ValueError(f"{name}: {len(sizes)} sizes for {B} images")
        for b, r in enumerate(rows):
            for i, e in enumerate(r):
                if [int(e["size"][0]), int(e["size"][1])] != [int(sizes[b][0]), int(sizes[b][1])]:
                    raise ValueError(f"{name}: RLE {i} of image {b} has size {list(e['size'])}, its image {list(sizes[b])}")
        runs = [np.ascontiguousarray(e["counts"], dtype=np.uint32).ravel() for r in rows for e in r]
        counts = np.concatenate(runs) if runs else np.zeros(0, np.uint32)
        offs = np.concatenate(([0], np.cumsum([len(c) for c in runs]))).astype(np.int64)
    if device is not None and isinstance(counts, np.ndarray):
        import torch
        counts = torch.from_numpy(np.ascontiguousarray(counts).view(np.int32).copy()).to(device)
        offs = torch.from_numpy(offs.copy()).to(device)
    return (addressable(counts), offs, B, slots, *sizes_of(sizes))


def is_pair(rle):
    """Did a (counts, run_offsets) pair come in, and not rows?"""
    return isinstance(rle, tuple) and len(rle) == 2 and not isinstance(rle[0], (list, tuple, dict))


def pair_device(rle):
    """The device of a (counts, run_offsets) pair of CUDA tensors; None for every other form."""
    return rle[0].device if is_pair(rle) and hasattr(rle[0], "is_cuda") else None


class RleSet:
    """The RLE set of one call, as rle_set normalises it: ``pair`` (did a (counts, run_offsets) pair come in), ``space`` (where the
    call runs), ``counts`` and ``offs`` there, ``B`` images of ``slots`` RLEs (``n`` in all), ``image_hs``, ``image_ws`` as the
    per-image entries take them, and on request image_sizes() and the per-RLE sides().

    device = None, and not the host definition: a pair of CUDA tensors runs where it lies, everything else on the host.  The entries
    whose detection rows decide pass the rows' device and in_place=False."""

    def __init__(self, name, rle, sizes, device, host_definition, in_place=True):
        self.pair, self.host_definition = is_pair(rle), host_definition
        if in_place and device is None and not host_definition and self.pair and hasattr(rle[0], "is_cuda"):
            device = rle[0].device
        self.counts, self.offs, self.B, self.slots, self.image_hs, self.image_ws = rle_set(name, rle, sizes, device)
        self.space = Space(device)
        self.n, self._sides = self.B * self.slots, None

    def image_sizes(self):
        """[(h_b, w_b)] per image"""
        return [(int(h), int(w)) for h, w in zip(self.image_hs, self.image_ws)]

    def sides(self):
        """(hs, ws) per RLE, int32, as the flat entries take them: made when first asked for, the per-image entries never do"""
        if self._sides is None:
            self._sides = np.repeat(self.image_hs, self.slots).astype(np.int32), np.repeat(self.image_ws, self.slots).astype(np.int32)
        return self._sides


def rle_results(space, B, per, hs, ws, capacity, call, resident=None):
    """The run lengths of B images x ``per`` RLEs: call(counts, capacity, run_offsets) -> status runs with a first guess of the
    capacity and, if the library answers MRCNN_ERR_SHAPE with the offsets complete (the capacity was the reason), once more with
    the need it reported.  Returns rles[b][i] = {"size": [h_b, w_b], "counts": uint32 runs}; only the used runs cross to the host.
    resident: a list that receives the (counts, run_offsets) pair as the library wrote it, in the call's own memory space."""
    n = max(0, B * per)
    offs_buf = space.new(n + 1, np.int64, zero=True)

    def attempt(capacity):
        counts = space.new(max(1, capacity), np.uint32)
        st = call(counts, capacity, offs_buf)
        offsets = space.host(offs_buf)
        return st, int(offsets[n]), (counts, offsets)
    counts, offsets = with_capacity(capacity, attempt)
    used = int(offsets[n])
    if resident is not None:
        resident.append((counts[:used], offs_buf))
    host = space.host(counts[:used]).view(np.uint32)
    return [[{"size": [int(hs[b]), int(ws[b])], "counts": host[int(offsets[b * per + i]):int(offsets[b * per + i + 1])]}
             for i in range(per)] for b in range(B)]


def with_capacity(capacity, attempt):
    """The capacity retry: attempt(capacity) allocates for a capacity, calls the entry and returns (status, need, result).  The first
    guess runs and, if the library answers MRCNN_ERR_SHAPE and needs more than it was given (the capacity was the reason), one more
    attempt with the need it reported.  capacity and need may be tuples, grown together.  Returns the result of the last attempt."""
    for _ in range(2):
        st, need, result = attempt(capacity)
        if st != 4 or (all(n <= c for n, c in zip(need, capacity)) if isinstance(need, tuple) else need <= capacity):
            break
        capacity = need
    _lib.check(st)
    return result


def rle_out(space, rows, capacity, call, written=None):
    """The outputs of an entry that returns ``rows`` RLEs with their areas and boxes, with the capacity retry on the run lengths:
    call(out_counts, capacity, out_run_offsets, areas, bboxes) -> status takes the five arguments these entries end on, addresses
    and all.  written() is the number of RLEs the call wrote where that is not ``rows``.  Returns (counts, run_offsets, areas,
    bboxes) cut to the used part."""
    ptr = space.ptr
    out_offs, areas, bboxes = space.new(rows + 1, np.int64, zero=True), space.new(max(1, rows), np.uint32), space.new((max(1, rows), 4), np.int32)

    def attempt(capacity):
        out = space.new(max(1, capacity), np.uint32)
        st = call(ptr(out), capacity, ptr(out_offs), ptr(areas), ptr(bboxes))
        m = rows if written is None else written()
        used = int(out_offs[m])
        return st, used, (out[:used], m)
    out, m = with_capacity(capacity, attempt)
    return out, out_offs[:m + 1], areas[:m], bboxes[:m]
