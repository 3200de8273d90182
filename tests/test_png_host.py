"""The PNG encoder's host definition (csrc/png_host.cpp behind mrcnn_png_encode_host) and the argument checks of the device entry:
no GPU.

tests/golden/png_v1.npz (make_png_golden.py) holds the cases' samples and the file each must become, byte for byte.  Those bytes come
from a sequential pure-Python restatement of the format, written from its description and RFC 1951's tables independently of the
C++; here the definition is held to them, to zlib's inflater and CRCs, and to PIL's reading of the files."""
import ctypes as C
import importlib
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import HAS_GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "png_v1.npz"))
NAMES = sorted(k[:-7] for k in GOLD.files if k.endswith("_pixels"))
OK, ERR_INVALID, ERR_HIP, ERR_SHAPE = 0, 1, 3, 4
GREY8, INSTANCE = 0, 1
PALETTE = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0)]          # red, blue, green, yellow: mrcnn_render_detections_source's


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


@pytest.fixture(scope="module")
def png():
    return importlib.import_module("mask-rcnn-coreml_amd.png")


def case(name):
    pixels, rows = np.ascontiguousarray(GOLD[name + "_pixels"]), int(GOLD[name + "_rows"])
    return pixels, (rows if pixels.dtype == np.int16 else None), GOLD[name + "_file"].tobytes()


def samples_of(pixels, rows):
    """The sample bytes the format defines, rebuilt in numpy."""
    if pixels.dtype == np.uint8:
        return pixels
    v = pixels.astype(np.int64)
    return np.where((v >= -1) & (v < rows), v + 1, 0).astype(np.uint8)


def raw_of(pixels, rows):
    s = samples_of(pixels, rows)
    return np.concatenate([np.zeros((s.shape[0], 1), np.uint8), s], axis=1).tobytes()


def chunks_of(data):
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(data)
    return out


def test_the_fixture_holds_the_cases():
    assert {"one_pixel", "one_block", "second_block", "zeros_2x4095", "three_rows", "runs", "random", "instance_255", "instance_1"} == set(NAMES)
    shape = {n: GOLD[n + "_pixels"].shape for n in NAMES}
    assert shape["one_pixel"] == (1, 1) and shape["one_block"] == (1, 4095) and shape["second_block"] == (1, 4096)
    assert shape["zeros_2x4095"] == (2, 4095) and not GOLD["zeros_2x4095_pixels"].any() and shape["three_rows"] == (3, 2047)
    row = GOLD["runs_pixels"][0]
    edges = np.flatnonzero(np.diff(row.astype(int)) != 0) + 1
    assert np.diff(np.concatenate([[0], edges, [row.size]])).tolist() == [1, 2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 519] and row[0] != 0
    assert shape["random"] == (70, 61) and GOLD["random_pixels"].max() >= 144               # 9-bit literals, two blocks
    m = GOLD["instance_255_pixels"]
    assert m.dtype == np.int16 and m.shape == (120, 200) and int(GOLD["instance_255_rows"]) == 255
    assert (m == -1).any() and (m == 254).any() and (m == 300).sum() == 1 and (m == -2).sum() == 1
    assert GOLD["instance_1_pixels"].dtype == np.int16 and int(GOLD["instance_1_rows"]) == 1
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "png_v1.npz")) < 64 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_the_definition_equals_the_restatements_bytes(png, name):
    pixels, rows, want = case(name)
    got = png.encode_host(pixels, rows)
    assert len(got) == len(want) and got == want, f"{name}: first difference at byte {next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), -1)}"


@pytest.mark.parametrize("name", NAMES)
def test_structure_crcs_and_the_inflated_stream(png, name):
    pixels, rows, _ = case(name)
    data = png.encode_host(pixels, rows)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    chunks = chunks_of(data)
    instance = pixels.dtype == np.int16
    assert [c[0] for c in chunks] == ([b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"] if instance else [b"IHDR", b"IDAT", b"IEND"])
    for kind, body, crc in chunks:
        assert zlib.crc32(kind + body) == crc, kind
    by = {c[0]: c[1] for c in chunks}
    h, w = pixels.shape
    assert by[b"IHDR"] == struct.pack(">IIBBBBB", w, h, 8, 3 if instance else 0, 0, 0, 0) and by[b"IEND"] == b""
    if instance:
        assert by[b"PLTE"] == bytes(3) + b"".join(bytes(PALETTE[(k - 1) % 4]) for k in range(1, rows + 1))
        assert by[b"tRNS"] == b"\0"
    idat = by[b"IDAT"]
    raw = raw_of(pixels, rows)
    assert idat[:2] == b"\x78\x01" and idat[-4:] == struct.pack(">I", zlib.adler32(raw))
    assert zlib.decompress(idat) == raw
    assert zlib.decompressobj(-15).decompress(idat[2:-4]) == raw                            # the bare deflate stream ends where the Adler-32 starts
    parsed = png.parse(data)
    assert all(ok for _, _, ok in parsed["chunks"]) and (parsed["height"], parsed["width"]) == (h, w) and not parsed["filters"].any()
    np.testing.assert_array_equal(parsed["scanlines"], samples_of(pixels, rows))


def test_the_blocks_are_fixed_huffman_and_4096_raw_bytes_long(png):
    """BTYPE 01 everywhere and BFINAL on the last block only, read off the first block's header; and the bit count of 8192 zeros,
    worked out by hand from RFC 1951's tables: two blocks, the second starting inside the run, no match running over the boundary."""
    one, two = png.encode_host(case("one_block")[0]), png.encode_host(case("second_block")[0])
    assert chunks_of(one)[1][1][2] & 7 == 0b011                                             # N = 4096, one block: BFINAL 1, BTYPE 01 (LSB first)
    assert chunks_of(two)[1][1][2] & 7 == 0b010                                             # N = 4097, two blocks: the first is not final
    zeros = png.encode_host(case("zeros_2x4095")[0])
    full, rest = 8 + 5, 8 + 5 + 5                                                           # (258, 1): symbol 285 + distance; (225 | 226, 1): symbol 283, 5 extra bits
    first = 3 + 8 + 15 * full + rest + 7                                                    # the literal 0 at p = 0, then 4095 = 15 x 258 + 225
    second = 3 + 15 * full + rest + 7                                                       # 4096 = 15 x 258 + 226, reaching back over the block's start
    assert len(chunks_of(zeros)[1][1]) == 2 + (first + second + 7) // 8 + 4


@pytest.mark.parametrize("name", NAMES)
def test_pil_reads_the_samples_and_the_palette(png, name):
    Image = pytest.importorskip("PIL.Image")
    pixels, rows, _ = case(name)
    im = Image.open(io.BytesIO(png.encode_host(pixels, rows)))
    im.load()
    assert im.size == (pixels.shape[1], pixels.shape[0])
    np.testing.assert_array_equal(np.array(im), samples_of(pixels, rows))
    if pixels.dtype == np.int16:
        assert im.mode == "P" and im.info["transparency"] == 0
        pal = im.getpalette()[:3 * (rows + 1)]
        assert pal == [0, 0, 0] + [c for k in range(1, rows + 1) for c in PALETTE[(k - 1) % 4]]
        rgba = np.array(im.convert("RGBA"))
        assert (rgba[..., 3] == np.where(samples_of(pixels, rows) == 0, 0, 255)).all()      # "no detection" is transparent, the rest opaque
    else:
        assert im.mode == "L"


def encode_status(L, pixels, h, w, fmt, rows, capacity, out=None):
    n = C.c_int64(-1)
    st = L.lib().mrcnn_png_encode_host(pixels.ctypes.data if pixels is not None else None, h, w, fmt, rows,
                                       out.ctypes.data if out is not None else None, capacity, C.byref(n))
    return st, int(n.value)


def test_capacity_protocol(L):
    pixels, rows, want = case("instance_255")
    h, w = pixels.shape
    st, need = encode_status(L, pixels, h, w, INSTANCE, rows, 0)
    assert st == OK and need == len(want)                            # out = NULL, capacity 0: the size query
    out = np.full(need + 8, 0xAB, np.uint8)
    st, n = encode_status(L, pixels, h, w, INSTANCE, rows, need - 1, out)
    assert st == ERR_SHAPE and n == need and (out == 0xAB).all()     # too small: the size needed, nothing written
    assert str(need).encode() in L.lib().mrcnn_last_error()
    st, n = encode_status(L, pixels, h, w, INSTANCE, rows, need, out)
    assert st == OK and n == need and out[:need].tobytes() == want and (out[need:] == 0xAB).all()      # the sentinel behind the file stands
    st, n = encode_status(L, pixels, h, w, INSTANCE, rows, 0, out)   # capacity 0 with a buffer: too small, not a query
    assert st == ERR_SHAPE and n == need


def test_encode_host_errors(L):
    px = np.zeros((4, 4), np.int16)
    out = np.zeros(4096, np.uint8)
    assert encode_status(L, None, 4, 4, GREY8, 0, 4096, out)[0] == ERR_INVALID
    assert encode_status(L, px, 4, 4, 2, 1, 4096, out)[0] == ERR_INVALID and encode_status(L, px, 4, 4, -1, 1, 4096, out)[0] == ERR_INVALID
    assert encode_status(L, px, 4, 4, GREY8, 0, 16, None)[0] == ERR_INVALID         # a capacity without a buffer
    assert L.lib().mrcnn_png_encode_host(px.ctypes.data, 4, 4, GREY8, 0, out.ctypes.data, 4096, None) == ERR_INVALID
    for h, w in [(0, 4), (4, 0), (32768, 4), (4, 32768), (-1, 4)]:
        assert encode_status(L, px, h, w, GREY8, 0, 4096, out)[0] == ERR_SHAPE
    for rows in (0, 256, -3):
        assert encode_status(L, px, 4, 4, INSTANCE, rows, 4096, out)[0] == ERR_SHAPE
        assert "rows" in L.lib().mrcnn_last_error().decode()
    assert not out.any()                                             # no error wrote anything
    grey = np.arange(16, dtype=np.uint8).reshape(4, 4)
    files = []
    for rows in (0, 256, -3, 77):                                    # rows is ignored for GREY8
        st, n = encode_status(L, grey, 4, 4, GREY8, rows, 4096, out)
        assert st == OK
        files.append(out[:n].tobytes())
    assert len(set(files)) == 1


def batch_status(L, images, fmt, rows, memspace=0, capacity=1 << 16, batch=None, null=None):
    table = (L.PngSource * max(1, len(images)))()
    for b, im in enumerate(images):
        table[b].pixels, table[b].height, table[b].width = (im[0].ctypes.data if im[0] is not None else None), im[1], im[2]
    out = np.zeros(max(capacity, 1), np.uint8)
    offs = np.full(len(images) + 1, -1, np.int64)
    st = L.lib().mrcnn_png_encode_batch(None if null == "images" else table, len(images) if batch is None else batch, memspace, fmt, rows,
                                        None if null == "out" else out.ctypes.data, capacity, None if null == "offsets" else offs.ctypes.data)
    return st, L.lib().mrcnn_last_error().decode(), out


def test_encode_batch_argument_errors_come_before_the_device(L):
    """Every argument error is raised whether or not there is a GPU, and names the offending image."""
    px = np.zeros((4, 4), np.int16)
    good = (px, 4, 4)
    for null in ("images", "out", "offsets"):
        assert batch_status(L, [good], INSTANCE, 5, null=null)[0] == ERR_INVALID
    assert batch_status(L, [good], 2, 5)[0] == ERR_INVALID and batch_status(L, [good], -1, 5)[0] == ERR_INVALID
    assert batch_status(L, [good], INSTANCE, 5, memspace=2)[0] == ERR_INVALID
    st, msg, _ = batch_status(L, [good, (None, 4, 4)], INSTANCE, 5)
    assert st == ERR_INVALID and "image 1" in msg
    for h, w in [(0, 4), (4, 0), (32768, 4), (4, 32768)]:
        st, msg, _ = batch_status(L, [good, good, (px, h, w)], INSTANCE, 5)
        assert st == ERR_SHAPE and "image 2" in msg
    for rows in (0, 256):
        st, msg, _ = batch_status(L, [good], INSTANCE, rows)
        assert st == ERR_SHAPE and "rows" in msg
    assert batch_status(L, [good], INSTANCE, 5, batch=0)[0] == ERR_SHAPE and batch_status(L, [good], INSTANCE, 5, batch=1025)[0] == ERR_SHAPE


def test_encode_batch_has_no_cpu_fallback(L, png):
    """Without a gfx950 device the device entry fails with MRCNN_ERR_HIP and writes nothing; with one it equals the definition."""
    pixels, rows, want = case("instance_1")
    st, msg, out = batch_status(L, [(pixels, pixels.shape[0], pixels.shape[1])], INSTANCE, rows)
    if HAS_GPU:
        assert st == OK and out[:len(want)].tobytes() == want
    else:
        assert st == ERR_HIP and "no CPU fallback" in msg and not out.any()
        with pytest.raises(L.MrcnnError) as e:
            png.encode_batch([pixels], rows=rows)
        assert e.value.code == ERR_HIP


def test_the_symbols_are_declared_bound_and_exported(L, png):
    hdr = open(os.path.join(ROOT, "include", "maskrcnn_hip.h")).read()
    lib = L.lib()
    for sym in ("mrcnn_png_encode_host", "mrcnn_png_encode_batch"):
        assert sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in hdr
        assert len(getattr(lib, sym).argtypes) == 8
    assert "#define MRCNN_PNG_BLOCK_BYTES 4096" in hdr and "#define MRCNN_PNG_MAX_BATCH 1024" in hdr and "mrcnn_png_source;" in hdr
    assert C.sizeof(L.PngSource) == 16 and png.BLOCK_BYTES == 4096
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    assert callable(png.encode_host) and callable(png.encode_batch) and callable(png.parse) and callable(models.MaskRCNN.instance_pngs)


def test_the_mirror_refuses_what_it_cannot_name(png):
    with pytest.raises(ValueError, match="rows"):
        png.encode_host(np.zeros((4, 4), np.int16))                  # an instance map needs rows
    with pytest.raises(ValueError, match="dtype"):
        png.encode_host(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        png.encode_host(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="one format"):
        png.encode_batch([np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int16)], rows=3)
    assert png.encode_batch([]) == []
    with pytest.raises(ValueError, match="signature"):
        png.parse(b"\xff\xd8\xff\xe0 not a png")


def test_the_c_example_builds_and_has_no_cpu_fallback(L, tmp_path):
    L.lib()                                                       # (the library must be there: a missing one is a failure, not a skip)
    from test_c_host import _build_example
    exe = _build_example(tmp_path, "maskrcnn_instance_png")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 64 and "out.png" in r.stderr
    if not HAS_GPU:                                               # (with one, tests/test_gpu_png.py runs it against the mirror)
        (tmp_path / "x.rgb").write_bytes(bytes(4 * 4 * 3))
        r = subprocess.run([exe, str(tmp_path), str(tmp_path / "x.rgb"), "4", "4", str(tmp_path / "o.png")], capture_output=True, text=True, timeout=120)
        assert r.returncode == ERR_HIP and "no CPU fallback" in r.stderr and not (tmp_path / "o.png").exists()
