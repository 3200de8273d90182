"""The entropy stage on the GPU (MRCNN_JPEG_ENTROPY_DEVICE; kernels_jpeg_entropy.hip): self-synchronising parallel Huffman decoding
behind mrcnn_jpeg_decode_batch_on / mrcnn_maskrcnn_predict_jpegs_on.  The expectation is the host decoder's — coefficients, bytes,
status and message — and every comparison is exact.  The step function these kernels run (csrc/jpeg_entropy.h) is held to the host
decoder on damaged input, under ASan + UBSan, by tests/test_jpeg_entropy_host.py, which needs no GPU; the damaged files here are a
handful of that test's cases: ordinary bad input that must come back as the host path's status and message.
ORDER: run `pytest -m "not gpu" tests/test_jpeg_entropy_host.py` first and this file only once it has passed — the damaged-input test
below hands the kernels streams on which the step function must already be known not to read or write out of bounds."""
import numpy as np
import pytest

import jpeg_entropy_cases as K
from jpeg_entropy_cases import DEVICE, HOST
from test_gpu_jpeg import DECODABLE, FOUR, GOLD, SENTINEL, data_of

pytestmark = pytest.mark.gpu

NAMES = sorted(K.files())
OK, ERR_IO, ERR_UNSUPPORTED = 0, 2, 5


@pytest.mark.parametrize("unit", [4, 16, 0])
def test_device_coefficients_equal_the_host_decoders_without_a_fallback(unit):
    f = K.files()
    for n in NAMES:
        st, msg, coef, stats = K.coefficients([f[n]], DEVICE, unit)
        assert st == OK, (n, msg)
        assert list(stats[:2]) == [1, 0], (n, unit, stats.tolist())
        assert np.array_equal(coef, K.host_coefficients([n])), (n, unit, int((coef != K.host_coefficients([n])).sum()))
    st, msg, coef, stats = K.coefficients([f[n] for n in NAMES], DEVICE, unit)
    assert st == OK, msg
    print(f"unit {unit or 128}: {int(stats[3])} units, most rounds of a workgroup {int(stats[2])}")
    assert list(stats[:2]) == [len(NAMES), 0], (unit, stats.tolist())
    assert np.array_equal(coef, K.host_coefficients(NAMES)), unit
    if unit == 4:                        # every file above 1 KB spans several workgroups of 256 four-byte units
        assert int(stats[3]) > 256 * 2 * sum(len(f[n]) > 2048 for n in NAMES)


def _ragged_call(files, sizes, device, entropy):
    import torch
    L = K._mod("_lib")
    table, keep = K._mod("jpeg").file_table(files)
    B = len(files)
    offsets = np.zeros(B, np.int64)
    total = 0
    for b, (h, w) in enumerate(sizes):
        offsets[b] = total
        total += (h * w * 3 + 15) // 16 * 16 + 16
    hs, ws = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    if device:
        buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptr = buf.data_ptr()
    else:
        buf = np.full(total, SENTINEL, np.uint8)
        ptr = buf.ctypes.data
    st = L.lib().mrcnn_jpeg_decode_batch_on(table, B, L.DEVICE if device else L.HOST, entropy, ptr, offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    msg = L.lib().mrcnn_last_error().decode() if st else ""
    del keep
    return st, msg, (buf.cpu().numpy() if device else buf), offsets


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_decode_batch_with_device_entropy_equals_libjpeg_and_writes_nothing_else(device):
    sizes = [tuple(int(v) for v in GOLD[n + "_info"][:2]) for n in DECODABLE]
    st, msg, buf, offsets = _ragged_call([data_of(n) for n in DECODABLE], sizes, device, DEVICE)
    assert st == OK, msg
    covered = np.zeros(buf.size, bool)
    for b, n in enumerate(DECODABLE):
        want = GOLD[n + "_rgb"]
        h, w = want.shape[:2]
        o = int(offsets[b])
        assert np.array_equal(buf[o:o + h * w * 3].reshape(h, w, 3), want), n
        covered[o:o + h * w * 3] = True
    assert (~covered).sum() >= 16 * len(DECODABLE) and (buf[~covered] == SENTINEL).all()
    images, got = K._mod("jpeg").decode_batch([data_of(n) for n in FOUR], device=device, entropy="device")
    for n, im in zip(FOUR, images):
        assert np.array_equal(im.cpu().numpy() if device else im, GOLD[n + "_rgb"]), n


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_refused_file_is_named_as_on_the_host_path_and_nothing_is_written(device):
    names = ["odd_420", "grey", "refused", "odd_444"]
    sizes = [tuple(int(v) for v in GOLD[n + "_info"][:2]) for n in names]
    want = _ragged_call([data_of(n) for n in names], sizes, device, HOST)
    got = _ragged_call([data_of(n) for n in names], sizes, device, DEVICE)
    assert got[0] == want[0] == ERR_UNSUPPORTED and got[1] == want[1] and "file 2 of the batch" in got[1] and "progressive" in got[1]
    assert (got[2] == SENTINEL).all()


def test_forced_fallback_and_damaged_files_get_the_host_paths_answer():
    f = K.files()
    # one round confirms nothing: every file of more than one unit goes through the host decoder, the result is the same
    st, msg, coef, stats = K.coefficients([f[n] for n in NAMES], DEVICE, 0, 1)
    assert st == OK, msg
    assert int(stats[1]) >= sum(len(f[n]) - 2 - K.scan_start(f[n]) > K.PRODUCTION_UNIT for n in NAMES) > 0 and int(stats[0]) + int(stats[1]) == len(NAMES)
    assert np.array_equal(coef, K.host_coefficients(NAMES))
    # ordinary bad inputs: a handful of the truncated / corrupted cases of the host test, alone and inside a batch
    seen = set()
    for name in ("restarts", "entropy_optimized", "entropy_restarts7"):
        cases = K.damaged(f[name], seed=len(f[name]))
        for label, bad in cases[1:5] + cases[5:9]:
            st_h, msg_h, coef_h, _ = K.coefficients([f["odd_420"], bad], HOST)
            st_d, msg_d, coef_d, _ = K.coefficients([f["odd_420"], bad], DEVICE)
            assert (st_d, msg_d) == (st_h, msg_h), (name, label)
            if st_h == OK:
                assert np.array_equal(coef_d, coef_h), (name, label)
            seen.add(st_h)
    assert ERR_IO in seen
    # and through the public entry: the host path's status and message
    bad = K.damaged(f["restarts"], seed=len(f["restarts"]))[2][1]
    sizes = [(35, 45), (70, 90)]
    want = _ragged_call([f["odd_420"], bad], sizes, False, HOST)
    got = _ragged_call([f["odd_420"], bad], sizes, False, DEVICE)
    assert got[0] == want[0] == ERR_IO and got[1] == want[1] and "file 1 of the batch" in got[1]


@pytest.fixture(scope="module")
def model(small_model):
    d, cfg = small_model
    return K._mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")


def test_predict_jpegs_with_device_entropy_equals_host_entropy(model):
    import torch
    files = [data_of(n) for n in FOUR]
    want_det, want_mask, want_sizes = model.predict_jpegs(files, entropy="host")
    det, mask, sizes = model.predict_jpegs(files, entropy="device")
    assert sizes == want_sizes and torch.equal(det, want_det) and torch.equal(mask, want_mask)
    assert float(det[..., 5].max()) > 0
    det1, mask1, sizes1 = model.predict_jpegs(files[2:3], entropy="device")          # a smaller batch right after, from the same staging
    assert sizes1 == sizes[2:3] and torch.equal(det1[0], want_det[2]) and torch.equal(mask1[0], want_mask[2])
    L = K._mod("_lib")
    with pytest.raises(L.MrcnnError) as e:
        model.predict_jpegs(files[:2] + [data_of("refused")], entropy="device")
    assert e.value.code == ERR_UNSUPPORTED and "file 2 of the batch" in str(e.value)
