"""The JPEG decoder's host half (csrc/jpeg_host.cpp behind mrcnn_jpeg_info / mrcnn_jpeg_decode_host): no GPU.

tests/golden/jpeg_v1.npz (make_jpeg_golden.py) holds small JPEG files and the RGB that PIL — libjpeg-turbo's default pipeline —
decodes from them.  Every step of that pipeline is integer arithmetic, so the bar is equality."""
import ctypes as C
import importlib
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import HAS_GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mask-rcnn-coreml_amd", "csrc")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_v1.npz"))
NAMES = sorted(k[:-4] for k in GOLD.files if k.endswith("_jpg"))
DECODABLE = [n for n in NAMES if n + "_rgb" in GOLD.files]
OK, ERR_IO, ERR_HIP, ERR_SHAPE, ERR_UNSUPPORTED = 0, 2, 3, 4, 5


def data_of(name):
    return GOLD[name + "_jpg"].tobytes()


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("mask-rcnn-coreml_amd._lib")


@pytest.fixture(scope="module")
def jpeg():
    return importlib.import_module("mask-rcnn-coreml_amd.jpeg")


def decode_status(L, data, capacity=None):
    """(status, rgb or None) of mrcnn_jpeg_decode_host with a buffer of the size the header names (or `capacity` bytes)."""
    a = np.frombuffer(data, np.uint8)
    v = [C.c_int32(0) for _ in range(5)]
    st = L.lib().mrcnn_jpeg_info(a.ctypes.data, a.size, *[C.byref(x) for x in v])
    if st != OK:
        return st, None
    h, w = v[0].value, v[1].value
    if h * w * 3 > 1 << 26:                                  # a corrupted size field
        return ERR_SHAPE, None
    n = h * w * 3 if capacity is None else capacity
    rgb = np.zeros(max(n, 1), np.uint8)
    st = L.lib().mrcnn_jpeg_decode_host(a.ctypes.data, a.size, rgb.ctypes.data, n)
    return st, (rgb[:h * w * 3].reshape(h, w, 3) if st == OK else None)


def test_the_fixture_holds_the_cases():
    assert len(NAMES) == 14 and len(DECODABLE) == 13 and "refused" not in DECODABLE
    assert {"one_pixel", "one_block", "one_over", "exact_mcu", "odd_444", "odd_422", "odd_420", "narrow", "custom_tables", "restarts",
            "coarse", "grey", "saturated", "refused"} == set(NAMES)


@pytest.mark.parametrize("name", DECODABLE)
def test_info_names_size_components_and_sampling(jpeg, name):
    h, w, comps, hs, vs = (int(v) for v in GOLD[name + "_info"])
    assert jpeg.info(data_of(name)) == {"height": h, "width": w, "components": comps, "h_samp": hs, "v_samp": vs}
    assert GOLD[name + "_rgb"].shape == (h, w, 3)


@pytest.mark.parametrize("name", DECODABLE)
def test_decode_host_equals_libjpeg(jpeg, name):
    got = jpeg.decode_host(data_of(name))
    want = GOLD[name + "_rgb"]
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"


def test_progressive_is_refused_by_name(L, jpeg):
    with pytest.raises(L.MrcnnError) as e:
        jpeg.info(data_of("refused"))
    assert e.value.code == ERR_UNSUPPORTED and "progressive" in str(e.value)
    with pytest.raises(L.MrcnnError) as e:
        jpeg.decode_host(data_of("refused"))
    assert e.value.code == ERR_UNSUPPORTED


def test_every_truncation_is_an_error(L):
    data = data_of("restarts")
    assert b"\xff\xdd" in data and b"\xff\xd0" in data            # DRI and RST0 are really there
    assert decode_status(L, data)[0] == OK
    for k in range(len(data)):
        st, _ = decode_status(L, data[:k])
        assert st in (ERR_IO, ERR_UNSUPPORTED), (k, st)


def test_corrupted_bytes_return_a_status(L):
    data = bytearray(data_of("restarts"))
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(200):
        at, flip = int(rng.integers(0, len(data))), int(rng.integers(1, 256))
        data[at] ^= flip
        st, _ = decode_status(L, bytes(data))
        data[at] ^= flip
        assert st in (0, 1, 2, 4, 5), (at, flip, st)
        seen.add(st)
    assert ERR_IO in seen                                         # some corruption is noticed as one


def test_capacity_one_byte_short(L):
    data = data_of("restarts")
    h, w = (int(v) for v in GOLD["restarts_info"][:2])
    assert decode_status(L, data, capacity=h * w * 3 - 1)[0] == ERR_SHAPE
    assert decode_status(L, data, capacity=h * w * 3)[0] == OK


def test_device_entries_have_no_cpu_fallback(L):
    if HAS_GPU:
        pytest.skip("GPU present: tests/test_gpu_jpeg.py runs the device entries")
    data = np.frombuffer(data_of("odd_420"), np.uint8)
    table = (L.Jpeg * 1)()
    table[0].data, table[0].length = data.ctypes.data, data.size
    out = np.zeros(35 * 45 * 3, np.uint8)
    off = np.zeros(1, np.int64)
    hs, ws = np.zeros(1, np.int32), np.zeros(1, np.int32)
    st = L.lib().mrcnn_jpeg_decode_batch(table, 1, L.HOST, out.ctypes.data, off.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    assert st == ERR_HIP and b"no CPU fallback" in L.lib().mrcnn_last_error() and not out.any()
    det, mask = np.zeros(6, np.float32), np.zeros(28 * 28, np.float32)
    st = L.lib().mrcnn_maskrcnn_predict_jpegs(None, table, 1, L.HOST, det.ctypes.data, mask.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    assert st == ERR_HIP and b"no CPU fallback" in L.lib().mrcnn_last_error()


def test_jpeg_c_host_builds_and_names_a_refused_file(L, tmp_path):
    L.lib()                                                       # (the library must be there: a missing one is a failure, not a skip)
    from test_c_host import _build_example
    exe = _build_example(tmp_path, "maskrcnn_predict_jpeg")
    (tmp_path / "p.jpg").write_bytes(data_of("refused"))
    r = subprocess.run([exe, str(tmp_path), str(tmp_path / "p.jpg")], capture_output=True, text=True, timeout=120)
    assert r.returncode == ERR_UNSUPPORTED and "progressive" in r.stderr and r.stdout == ""
    if not HAS_GPU:
        (tmp_path / "q.jpg").write_bytes(data_of("odd_420"))
        r = subprocess.run([exe, str(tmp_path), str(tmp_path / "q.jpg")], capture_output=True, text=True, timeout=120)
        assert r.returncode == ERR_HIP and "no CPU fallback" in r.stderr and r.stdout == ""


def test_the_parser_is_clean_under_the_sanitizers(tmp_path):
    """tools/jpeg_host_check.cpp, a program of its own built from jpeg_host.cpp with ASan + UBSan: every fixture, every truncation,
    200 seeded corruptions each.  Skips only where the compiler has no sanitizer runtime."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no sanitizer runtime here")
    exe = str(tmp_path / "jpeg_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", CSRC, os.path.join(ROOT, "tools", "jpeg_host_check.cpp"),
                        os.path.join(CSRC, "jpeg_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = tmp_path / "files"
    files.mkdir()
    for name in NAMES:
        (files / (name + ".jpg")).write_bytes(data_of(name))
    r = subprocess.run([exe, str(files)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 findings" in r.stdout


def test_the_host_decoder_answers_what_it_always_answered(L):
    """tests/golden/jpeg_host_answers_v1.npz (make_jpeg_host_answers.py): status, message and the CRC32 of the coefficients that
    mrcnn_jpeg_coefficients(entropy = HOST) gave on the 25 files of jpeg_entropy_cases.py, intact and in their 25 damaged variants
    each, recorded from the commit before the decoder's tables and lookup were shared.  650 answers, equal case by case."""
    import sys
    import jpeg_entropy_cases as K
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        maker = importlib.import_module("make_jpeg_host_answers")
    finally:
        sys.path.pop(0)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_host_answers_v1.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 64 * 1024 and gold["status"].shape == (25, 26) and len(gold["messages"]) == 168
    rows = maker.answers(K)
    assert [n for n, _ in rows] == gold["names"].tolist()
    for i, (name, row) in enumerate(rows):
        assert len(row) == 26
        for j, (label, st, msg, crc) in enumerate(row):
            want_st, want_msg, want_crc = int(gold["status"][i, j]), str(gold["messages"][gold["message"][i, j]]), int(gold["crc"][i, j])
            assert (st, msg, crc) == (want_st, want_msg, want_crc), \
                f"{name}, {label}: status {st} {msg!r} crc {crc:08x}; recorded: status {want_st} {want_msg!r} crc {want_crc:08x}"


def test_the_fixture_is_still_what_pil_decodes():
    Image = pytest.importorskip("PIL.Image")
    for name in DECODABLE:
        assert np.array_equal(np.array(Image.open(io.BytesIO(data_of(name))).convert("RGB")), GOLD[name + "_rgb"]), name
