"""The self-synchronising entropy stage without a GPU: the sequential host model of the device phases (csrc/jpeg_entropy_host.cpp, the
step function of csrc/jpeg_entropy.h that the kernels run too) against the host decoder, through mrcnn_jpeg_coefficients.  The bar is
equality: of the coefficients on intact files, with NO fallback, and of status and message on damaged ones."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_entropy_cases as K
from jpeg_entropy_cases import HOST, MODEL, ROOT

CSRC = os.path.join(ROOT, "mask-rcnn-coreml_amd", "csrc")
NAMES = sorted(K.files())
OK, ERR_INVALID, ERR_IO, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 4, 5


def test_the_fixtures_hold_the_cases_and_the_stuffed_bytes_at_unit_ends():
    f = K.files()
    assert len(NAMES) == 25 and {"entropy_tail_rst", "entropy_tail_eoi", "entropy_flat_grey", "entropy_flat_128", "entropy_flat_77", "entropy_flat_128_rst", "entropy_flat_77_rst", "one_pixel", "restarts", "saturated", "entropy_restarts7", "entropy_optimized", "entropy_h2v1", "entropy_grey", "large"} <= set(NAMES)
    assert sum(v.size for k, v in K.GOLD2.items() if k.endswith("_jpg")) < 64 * 1024 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_entropy_v1.npz")) < 64 * 1024
    assert len(f["one_pixel"]) - 2 - K.scan_start(f["one_pixel"]) == 8                    # a scan shorter than any unit but the smallest
    r7 = f["entropy_restarts7"]
    assert sum(r7.count(bytes([0xFF, 0xD0 + k])) >= 1 for k in range(8)) == 8 and b"\xff\xdd\x00\x04\x00\x07" in r7
    assert 50_000 < len(f["large"]) < 64_000 and (len(f["large"]) - K.scan_start(f["large"])) // K.PRODUCTION_UNIT > 256     # more than one workgroup of units
    # a segment whose last data byte is an FF: its stuffed 00 stands directly in front of the marker, with DRI and without
    rst, eoi = f["entropy_tail_rst"], f["entropy_tail_eoi"]
    assert any(bytes([0xFF, 0x00, 0xFF, 0xD0 + k]) in rst[K.scan_start(rst):] for k in range(8)) and b"\xff\xdd" in rst[:K.scan_start(rst)]
    assert any(t % 4 == 3 for t in K.stuffed_tails(rst)[:-1])       # ... and once the FF closes a 4-byte unit: the stuffed 00 opens the segment's last unit alone
    assert eoi.endswith(b"\xff\x00\xff\xd9") and b"\xff\xdd" not in eoi[:K.scan_start(eoi)]
    # the precondition: a stuffed FF 00 whose FF is the last byte of a unit, at every unit size the tests run
    for unit in (4, 16):
        assert sum(K.stuffed_at_unit_end(f[n], unit) for n in NAMES) >= 1, unit
    assert K.stuffed_at_unit_end(f["large"], K.PRODUCTION_UNIT) >= 1


@pytest.mark.parametrize("unit", [4, 16, 128, 0])
def test_the_model_equals_the_host_decoder_without_a_fallback(unit):
    f = K.files()
    for n in NAMES:
        st, msg, coef, stats = K.coefficients([f[n]], MODEL, unit)
        assert st == OK, (n, msg)
        assert list(stats[:2]) == [1, 0], (n, unit, stats.tolist())
        assert np.array_equal(coef, K.host_coefficients([n])), (n, unit)
    for batch in (NAMES, NAMES[::-1][:7], ["large", "one_pixel", "restarts", "large"]):
        st, msg, coef, stats = K.coefficients([f[n] for n in batch], MODEL, unit)
        assert st == OK, msg
        assert list(stats[:2]) == [len(batch), 0], (unit, stats.tolist())
        assert np.array_equal(coef, K.host_coefficients(batch)), unit
        print(f"unit {unit or 128}: batch of {len(batch)}: {int(stats[3])} units, most rounds of a workgroup {int(stats[2])}")


def test_one_round_cannot_confirm_a_state_so_every_multi_unit_file_falls_back():
    f = K.files()
    for unit in (16, 0):
        U = unit or K.PRODUCTION_UNIT
        multi = [n for n in NAMES if len(f[n]) - 2 - K.scan_start(f[n]) > U]
        single = [n for n in NAMES if n not in multi]
        assert multi and (single or unit == 16)
        st, msg, coef, stats = K.coefficients([f[n] for n in NAMES], MODEL, unit, 1)
        assert st == OK, msg
        assert int(stats[1]) >= len(multi) and int(stats[0]) + int(stats[1]) == len(NAMES), stats.tolist()
        assert np.array_equal(coef, K.host_coefficients(NAMES))
        for n in multi[:4] + multi[-2:]:
            st, msg, coef, stats = K.coefficients([f[n]], MODEL, unit, 1)
            assert st == OK and list(stats[:2]) == [0, 1] and np.array_equal(coef, K.host_coefficients([n])), (n, stats.tolist())


@pytest.mark.parametrize("name", NAMES)
def test_damaged_files_get_the_host_decoders_status_and_message(name):
    data = K.files()[name]
    cases = K.damaged(data, seed=len(data))
    assert len(cases) == 25
    seen = set()
    for unit in (16, 0):
        for label, bad in cases:
            st_h, msg_h, coef_h, _ = K.coefficients([bad], HOST)
            st_m, msg_m, coef_m, stats = K.coefficients([bad], MODEL, unit)
            assert (st_m, msg_m) == (st_h, msg_h), (name, label, unit)
            if st_h == OK:
                assert np.array_equal(coef_m, coef_h), (name, label, unit)
            seen.add(st_h)
    assert ERR_IO in seen
    # in a batch the damaged file is named by its index, as the host path names it
    good = K.files()["odd_420"]
    st_h, msg_h, _, _ = K.coefficients([good, cases[2][1], good], HOST)
    st_m, msg_m, _, _ = K.coefficients([good, cases[2][1], good], MODEL)
    assert st_h == ERR_IO and "file 1 of the batch" in msg_h and (st_m, msg_m) == (st_h, msg_h)


def test_the_model_is_clean_under_the_sanitizers(tmp_path):
    """tools/jpeg_entropy_check.cpp, a program of its own built from jpeg_entropy_host.cpp and jpeg_host.cpp with ASan + UBSan: every
    fixture file (the flat ones, whose intervals end on blocks shorter than padding, included), its truncations (every one; every third
    for a file above 16 KB), 200 seeded corruptions each, unit sizes 4, 16 and 128, exact-size buffers.  Nothing sanitised is loaded
    into Python.  Only `large`, generated here and no fixture, is left out."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]     # (no sanitizer runtime is a failure here: the GPU tests rest on this proof)
    exe = str(tmp_path / "jpeg_entropy_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", CSRC, os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"),
                        os.path.join(CSRC, "jpeg_entropy_host.cpp"), os.path.join(CSRC, "jpeg_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = tmp_path / "files"
    files.mkdir()
    for name, data in K.files().items():
        if name != "large":
            (files / (name + ".jpg")).write_bytes(data)
    (files / "refused.jpg").write_bytes(K.GOLD1["refused_jpg"].tobytes())
    r = subprocess.run([exe, str(files)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 findings" in r.stdout


def test_bad_entropy_and_bad_knobs_are_refused():
    L, J = K._mod("_lib"), K._mod("jpeg")
    data = K.files()["odd_420"]
    for entropy in (-1, 3):
        assert K.coefficients([data], entropy)[0] == ERR_INVALID
    for unit in (-4, 2, 3, 24, 2048):
        st, msg, _, _ = K.coefficients([data], MODEL, unit)
        assert st == ERR_INVALID and "unit_bytes" in msg, unit
    assert K.coefficients([data], MODEL, 0, -1)[0] == ERR_INVALID
    # the two public entries refuse an unknown entropy value before anything else, with or without a GPU
    table, keep = J.file_table([data])
    out, off = np.zeros(35 * 45 * 3, np.uint8), np.zeros(1, np.int64)
    hs, ws = np.zeros(1, np.int32), np.zeros(1, np.int32)
    st = L.lib().mrcnn_jpeg_decode_batch_on(table, 1, L.HOST, 2, out.ctypes.data, off.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    assert st == ERR_INVALID and b"entropy 2" in L.lib().mrcnn_last_error() and not out.any()
    det, mask = np.zeros(6, np.float32), np.zeros(28 * 28, np.float32)
    st = L.lib().mrcnn_maskrcnn_predict_jpegs_on(None, table, 1, L.HOST, 7, det.ctypes.data, mask.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    assert st == ERR_INVALID and b"entropy 7" in L.lib().mrcnn_last_error()
    with pytest.raises(ValueError):
        J.decode_batch([data], entropy="gpu")
    # capacity one coefficient short
    block0, stats = np.zeros(2, np.int64), np.zeros(4, np.int32)
    coef = np.zeros(1 << 16, np.int16)
    assert L.lib().mrcnn_jpeg_coefficients(table, 1, HOST, 0, 0, coef.ctypes.data, 0, block0.ctypes.data, stats.ctypes.data) == ERR_SHAPE
    need = int(block0[1]) * 64
    assert L.lib().mrcnn_jpeg_coefficients(table, 1, HOST, 0, 0, coef.ctypes.data, need - 1, block0.ctypes.data, stats.ctypes.data) == ERR_SHAPE
    assert L.lib().mrcnn_jpeg_coefficients(table, 1, HOST, 0, 0, coef.ctypes.data, need, block0.ctypes.data, stats.ctypes.data) == OK
    del keep


def test_the_knobs_are_armed_only_for_tests():
    """unit_bytes / max_rounds in a process without MRCNN_TEST_KNOBS=1: MRCNN_ERR_UNSUPPORTED; the production values work there."""
    import sys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import jpeg_entropy_cases as K\n"
            "d = K.files()['odd_420']\n"
            "print(K.coefficients([d], 2, 16)[0], K.coefficients([d], 2, 0, 3)[0], K.coefficients([d], 2)[0])\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if k != "MRCNN_TEST_KNOBS"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.split() == ["5", "5", "0"], r.stdout + r.stderr


def test_a_file_of_many_workgroups_converges_within_the_launch_cap():
    """The production launch count is capped from the files' sizes (jpeg_entropy.h ent_launches: a wrong state may cross 64 KB of stream, 4
    launches at 128-byte units).  A 960x1280 noise-on-gradient file of about 870 KB — 27 workgroups of production units — must still
    decode clean: states resynchronise inside a workgroup, so the cap does not grow with the file."""
    import importlib, sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        maker = importlib.import_module("make_jpeg_entropy_golden_images")
    finally:
        sys.path.pop(0)
    big = K._mod("jpeg").encode_host(maker.synthetic(960, 1280, "RGB", np.random.default_rng(5)), 90, "420")
    assert len(big) > 800_000
    st_h, msg, want, _ = K.coefficients([big], HOST)
    st_m, msg, got, stats = K.coefficients([big], MODEL)
    assert st_h == st_m == OK, msg
    assert list(stats[:2]) == [1, 0] and int(stats[3]) > 25 * 256, stats.tolist()
    assert np.array_equal(got, want)
