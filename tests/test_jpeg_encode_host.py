"""The JPEG encoder's host definition (csrc/jpeg_enc_host.cpp behind mrcnn_jpeg_encode_host) and the argument checks of the device
entry: no GPU.

tests/golden/jpeg_enc_v1.npz (make_jpeg_enc_golden.py) holds source pixels and the RGB that PIL decodes from PIL's own encoding of
them at the same quality and sampling.  The project's decoder equals libjpeg byte for byte (tests/test_jpeg_host.py), and every step
of libjpeg's default compressor is integer arithmetic, so decode_host(encode_host(pixels)) is held to EQUALITY with that RGB: the
encoder's tables and coefficients are libjpeg's on every visible sample.  (Measured when the fixture was made: 0 differing bytes in
all four sampling modes, so no mode carries a stored tolerance.)"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import HAS_GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_enc_v1.npz"))
NAMES = sorted(k[:-7] for k in GOLD.files if k.endswith("_pixels"))
OK, ERR_INVALID, ERR_HIP, ERR_SHAPE = 0, 1, 3, 4
SAMPLING_FACTORS = {0: (3, 1, 1), 1: (3, 2, 1), 2: (3, 2, 2), 3: (1, 1, 1)}      # components, h_samp, v_samp as mrcnn_jpeg_info reports them


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


@pytest.fixture(scope="module")
def jpeg():
    return importlib.import_module("mask-rcnn-coreml_amd.jpeg")


def case(name):
    quality, sampling = (int(v) for v in GOLD[name + "_params"])
    return np.ascontiguousarray(GOLD[name + "_pixels"]), quality, sampling, GOLD[name + "_ref"]


def encode_status(L, rgb, h, w, quality, sampling, capacity, out=None):
    n = C.c_int64(-1)
    st = L.lib().mrcnn_jpeg_encode_host(rgb.ctypes.data if rgb is not None else None, h, w, quality, sampling,
                                        out.ctypes.data if out is not None else None, capacity, C.byref(n))
    return st, int(n.value)


def test_the_fixture_holds_the_cases():
    assert {"one_pixel", "one_block", "one_over", "exact_mcu", "odd_444", "odd_422", "odd_420", "even_420", "narrow", "coarse", "grey",
            "saturated", "flat", "zrl", "pad_ff"} == set(NAMES)
    shapes = {n: (GOLD[n + "_pixels"].shape[:2], tuple(int(v) for v in GOLD[n + "_params"])) for n in NAMES}
    assert shapes["one_pixel"][0] == (1, 1) and shapes["one_block"][0] == (8, 8) and shapes["one_over"][0] == (9, 9)
    assert shapes["exact_mcu"][0] == (16, 16)
    assert shapes["odd_444"] == ((17, 23), (90, 0)) and shapes["odd_422"][0] == (33, 47) and shapes["odd_422"][1][1] == 1
    assert shapes["odd_420"][0] == (35, 45) and shapes["odd_420"][1][1] == 2
    assert shapes["narrow"] == ((31, 9), (100, 2)) and shapes["coarse"] == ((40, 40), (3, 2))
    assert shapes["grey"][0] == (40, 40) and shapes["grey"][1][1] == 3
    assert shapes["saturated"] == ((24, 24), (100, 0)) and shapes["flat"][0] == (32, 32) and shapes["zrl"][0] == (32, 32)
    assert not [k for k in GOLD.files if k.endswith("_tol")]          # no sampling mode needed a tolerance


@pytest.mark.parametrize("name", NAMES)
def test_decoding_our_file_equals_libjpegs_own_round_trip(jpeg, name):
    pixels, quality, sampling, want = case(name)
    data = jpeg.encode_host(pixels, quality, sampling)
    assert data[:4] == b"\xff\xd8\xff\xe0" and data[6:11] == b"JFIF\0" and data[-2:] == b"\xff\xd9"
    got = jpeg.decode_host(data)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ, max {int(np.abs(got.astype(int) - want.astype(int)).max())}"


@pytest.mark.parametrize("name", NAMES)
def test_info_reports_size_components_and_sampling(jpeg, name):
    pixels, quality, sampling, _ = case(name)
    comps, hs, vs = SAMPLING_FACTORS[sampling]
    assert jpeg.info(jpeg.encode_host(pixels, quality, sampling)) == {"height": pixels.shape[0], "width": pixels.shape[1], "components": comps,
                                                                      "h_samp": hs, "v_samp": vs}


def test_the_set_exercises_stuffing_and_the_padded_ff(jpeg):
    scans = {}
    for name in NAMES:
        pixels, quality, sampling, _ = case(name)
        data = jpeg.encode_host(pixels, quality, sampling)
        scans[name] = data[data.index(b"\xff\xda") + 2 + ((data[data.index(b"\xff\xda") + 2] << 8) | data[data.index(b"\xff\xda") + 3]):-2]
    assert sum(s.count(b"\xff\x00") for s in scans.values()) >= 10
    assert scans["pad_ff"].endswith(b"\xff\x00")                    # the last byte, 1-padding included, is an FF and is stuffed
    for name, s in scans.items():                                   # an FF in a scan is always followed by 00: no marker inside
        assert s.count(b"\xff") == s.count(b"\xff\x00"), name


def test_markers_come_in_the_documented_order(jpeg):
    pixels, quality, sampling, _ = case("odd_420")
    data = jpeg.encode_host(pixels, quality, sampling)
    pos, seen = 2, []
    while True:
        assert data[pos] == 0xFF
        seen.append(data[pos + 1])
        if data[pos + 1] == 0xDA:
            break
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    assert seen == [0xE0, 0xDB, 0xC0, 0xC4, 0xDA]
    assert data[11:20] == bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])        # JFIF 1.1, no units, density 1:1, no thumbnail


@pytest.mark.parametrize("quality,first_luma,last_luma", [(1, 255, 255), (50, 16, 99), (100, 1, 1)])
def test_quality_scales_annex_k_and_clamps(jpeg, quality, first_luma, last_luma):
    """libjpeg's rule on Annex K's luminance table (16 .. 99): q1 scales by 50 and clamps to 255, q50 is the table itself, q100 clamps to 1."""
    pixels, _, _, _ = case("odd_444")
    data = jpeg.encode_host(pixels, quality, 0)
    at = data.index(b"\xff\xdb")
    table = data[at + 5:at + 5 + 64]                                # zigzag order: first and last entries are those of the natural order
    assert (table[0], table[63]) == (first_luma, last_luma)
    assert min(table) >= 1 and max(table) <= 255
    assert jpeg.decode_host(data).shape == pixels.shape            # (the clamped tables still make a decodable file)


def test_capacity_protocol(L):
    pixels, quality, sampling, _ = case("odd_420")
    h, w = pixels.shape[:2]
    st, need = encode_status(L, pixels, h, w, quality, sampling, 0)
    assert st == OK and need > 600                                   # out = NULL, capacity 0: the size query
    out = np.full(need + 8, 0xAB, np.uint8)
    st, n = encode_status(L, pixels, h, w, quality, sampling, need - 1, out)
    assert st == ERR_SHAPE and n == need and (out == 0xAB).all()     # too small: the size needed, nothing written
    assert str(need).encode() in L.lib().mrcnn_last_error()
    st, n = encode_status(L, pixels, h, w, quality, sampling, need, out)
    assert st == OK and n == need and out[:2].tobytes() == b"\xff\xd8" and out[need - 2:need].tobytes() == b"\xff\xd9" and (out[need:] == 0xAB).all()
    st, n = encode_status(L, pixels, h, w, quality, sampling, 0, out)           # capacity 0 with a buffer: too small, not a query
    assert st == ERR_SHAPE and n == need


def test_encode_host_errors(L):
    px = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros(4096, np.uint8)
    assert encode_status(L, None, 4, 4, 90, 2, 4096, out)[0] == ERR_INVALID
    assert encode_status(L, px, 4, 4, 90, 4, 4096, out)[0] == ERR_INVALID and encode_status(L, px, 4, 4, 90, -1, 4096, out)[0] == ERR_INVALID
    assert encode_status(L, px, 4, 4, 90, 2, 16, None)[0] == ERR_INVALID          # a capacity without a buffer
    assert L.lib().mrcnn_jpeg_encode_host(px.ctypes.data, 4, 4, 90, 2, out.ctypes.data, 4096, None) == ERR_INVALID
    for h, w in [(0, 4), (4, 0), (32768, 4), (4, 32768), (-1, 4)]:
        assert encode_status(L, px, h, w, 90, 2, 4096, out)[0] == ERR_SHAPE
    for q in (0, 101, -5):
        assert encode_status(L, px, 4, 4, q, 2, 4096, out)[0] == ERR_SHAPE
    assert not out.any()


def batch_status(L, images, quality, sampling, memspace=0, capacity=1 << 16, batch=None, null=None):
    table = (L.Image * max(1, len(images)))()
    for b, im in enumerate(images):
        table[b].rgb, table[b].height, table[b].width = (im[0].ctypes.data if im[0] is not None else None), im[1], im[2]
    out = np.zeros(max(capacity, 1), np.uint8)
    offs = np.full(len(images) + 1, -1, np.int64)
    st = L.lib().mrcnn_jpeg_encode_batch(None if null == "images" else table, len(images) if batch is None else batch, memspace, quality, sampling,
                                         None if null == "out" else out.ctypes.data, capacity, None if null == "offsets" else offs.ctypes.data)
    return st, L.lib().mrcnn_last_error().decode(), out


def test_encode_batch_argument_errors_come_before_the_device(L):
    """Every argument error is raised whether or not there is a GPU, and names the offending image."""
    px = np.zeros((4, 4, 3), np.uint8)
    good = (px, 4, 4)
    for null in ("images", "out", "offsets"):
        assert batch_status(L, [good], 90, 2, null=null)[0] == ERR_INVALID
    assert batch_status(L, [good], 90, 4)[0] == ERR_INVALID and batch_status(L, [good], 90, -1)[0] == ERR_INVALID
    assert batch_status(L, [good], 90, 2, memspace=2)[0] == ERR_INVALID
    st, msg, _ = batch_status(L, [good, (None, 4, 4)], 90, 2)
    assert st == ERR_INVALID and "image 1" in msg
    for h, w in [(0, 4), (4, 0), (32768, 4), (4, 32768)]:
        st, msg, _ = batch_status(L, [good, good, (px, h, w)], 90, 2)
        assert st == ERR_SHAPE and "image 2" in msg
    for q in (0, 101):
        assert batch_status(L, [good], q, 2)[0] == ERR_SHAPE
    assert batch_status(L, [good], 90, 2, batch=0)[0] == ERR_SHAPE and batch_status(L, [good], 90, 2, batch=1025)[0] == ERR_SHAPE


def test_encode_batch_has_no_cpu_fallback(L, jpeg):
    """Without a gfx950 device the device entry fails with MRCNN_ERR_HIP and writes nothing; with one it equals the definition."""
    pixels, quality, sampling, _ = case("odd_420")
    st, msg, out = batch_status(L, [(pixels, pixels.shape[0], pixels.shape[1])], quality, sampling)
    if HAS_GPU:
        want = jpeg.encode_host(pixels, quality, sampling)
        assert st == OK and out[:len(want)].tobytes() == want
    else:
        assert st == ERR_HIP and "no CPU fallback" in msg and not out.any()


def test_the_c_example_builds_and_has_no_cpu_fallback(L, tmp_path):
    import subprocess
    L.lib()                                                       # (the library must be there: a missing one is a failure, not a skip)
    from test_c_host import _build_example
    exe = _build_example(tmp_path, "maskrcnn_render_jpeg")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 64 and "out.jpg" in r.stderr
    if not HAS_GPU:                                               # (with one, tests/test_gpu_jpeg_encode.py runs it against the mirror)
        (tmp_path / "x.rgb").write_bytes(bytes(4 * 4 * 3))
        r = subprocess.run([exe, str(tmp_path), str(tmp_path / "x.rgb"), "4", "4", str(tmp_path / "o.jpg")], capture_output=True, text=True, timeout=120)
        assert r.returncode == ERR_HIP and "no CPU fallback" in r.stderr and not (tmp_path / "o.jpg").exists()
