"""JPEG decode on the GPU (mrcnn_jpeg_decode_batch, mrcnn_maskrcnn_predict_jpegs; kernels_jpeg.hip): the entropy decoder on the
host, dequantisation + inverse DCT + chroma upsampling + colour conversion in two launches for a ragged batch.  The expectation is
tests/golden/jpeg_v1.npz — what PIL (libjpeg-turbo's defaults) decodes from the same bytes — and every comparison is exact."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_v1.npz"))
DECODABLE = sorted(k[:-4] for k in GOLD.files if k.endswith("_rgb"))
SENTINEL = 0xA5
ERR_UNSUPPORTED = 5


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def data_of(name):
    return GOLD[name + "_jpg"].tobytes()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", DECODABLE)
def test_each_file_alone_equals_libjpeg(name, device):
    images, sizes = _mod("jpeg").decode_batch([data_of(name)], device=device)
    want = GOLD[name + "_rgb"]
    got = images[0].cpu().numpy() if device else images[0]
    assert sizes == [want.shape[:2]] and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"


def _ragged_call(names, device):
    """One mrcnn_jpeg_decode_batch over `names` into a sentinel-filled buffer with a 16-byte gap behind every image →
    (status, the buffer on the host, offsets, heights, widths)."""
    import torch
    L = _mod("_lib")
    table, keep = _mod("jpeg").file_table([data_of(n) for n in names])
    B = len(names)
    offsets = np.zeros(B, np.int64)
    total = 0
    for b, n in enumerate(names):
        h, w = (int(v) for v in GOLD[n + "_info"][:2])
        offsets[b] = total
        total += (h * w * 3 + 15) // 16 * 16 + 16
    hs, ws = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    if device:
        buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptr = buf.data_ptr()
    else:
        buf = np.full(total, SENTINEL, np.uint8)
        ptr = buf.ctypes.data
    st = L.lib().mrcnn_jpeg_decode_batch(table, B, L.DEVICE if device else L.HOST, ptr, offsets.ctypes.data, hs.ctypes.data, ws.ctypes.data)
    del keep
    return st, (buf.cpu().numpy() if device else buf), offsets, hs, ws


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_ragged_batch_of_all_of_them(device):
    st, buf, offsets, hs, ws = _ragged_call(DECODABLE, device)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    covered = np.zeros(buf.size, bool)
    for b, n in enumerate(DECODABLE):
        want = GOLD[n + "_rgb"]
        h, w = want.shape[:2]
        assert (int(hs[b]), int(ws[b])) == (h, w), n
        o = int(offsets[b])
        assert np.array_equal(buf[o:o + h * w * 3].reshape(h, w, 3), want), n
        covered[o:o + h * w * 3] = True
    assert (~covered).sum() >= 16 * len(DECODABLE)                       # the gaps, and the one behind the last image
    assert (buf[~covered] == SENTINEL).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_refused_file_is_named_and_nothing_is_written(device):
    st, buf, _, _, _ = _ragged_call(["odd_420", "grey", "refused", "odd_444"], device)
    msg = _mod("_lib").lib().mrcnn_last_error().decode()
    assert st == ERR_UNSUPPORTED and "2" in msg and "file 2 of the batch" in msg and "progressive" in msg
    assert (buf == SENTINEL).all()


def test_bad_arguments():
    L, J = _mod("_lib"), _mod("jpeg")
    table, keep = J.file_table([data_of("odd_420"), data_of("grey")])
    out = np.zeros(1 << 15, np.uint8)
    hs, ws = np.zeros(2, np.int32), np.zeros(2, np.int32)

    def call(batch, offsets, out_ptr=out.ctypes.data):
        off = np.asarray(offsets, np.int64)
        return L.lib().mrcnn_jpeg_decode_batch(table, batch, L.HOST, out_ptr, off.ctypes.data, hs.ctypes.data, ws.ctypes.data)

    assert call(2, [0, 8192]) == 0
    assert call(2, [0, 8200]) == 1                      # not a multiple of 16
    assert call(2, [0, 4720]) == 1                      # 35*45*3 = 4725 bytes: the second image starts inside the first
    assert call(2, [4800, 16]) == 1                     # 40*40*3 = 4800 bytes from 16: the second image ends inside the first
    assert call(2, [0, 8192], None) == 1                # null output
    assert call(0, [0, 8192]) == 4 and call(1025, [0, 8192]) == 4
    assert not out[8192 + 40 * 40 * 3:].any()


FOUR = ["restarts", "odd_422", "grey", "narrow"]        # 70x90 4:2:0 with restarts, 33x47 4:2:2, 40x40 grey, 31x9 4:2:0


@pytest.fixture(scope="module")
def model(small_model):
    d, cfg = small_model
    return _mod("models").load_maskrcnn(d, max_batch=4, compute_dtype="f32x3")


def test_predict_jpegs_equals_predict_images_on_the_decoded_files(model):
    import torch
    J = _mod("jpeg")
    files = [data_of(n) for n in FOUR]
    det, mask, sizes = model.predict_jpegs(files)
    decoded = [J.decode_host(f) for f in files]
    assert sizes == [im.shape[:2] for im in decoded] and len({s for s in sizes}) == 4
    want_det, want_mask = model.predict_images([torch.from_numpy(im).cuda() for im in decoded])
    assert det.is_cuda and mask.is_cuda
    assert torch.equal(det, want_det) and torch.equal(mask, want_mask)
    assert float(det[..., 5].max()) > 0                                  # there are detections to compare
    # a smaller batch right after, from the same staging; and the batch limit
    det1, mask1, sizes1 = model.predict_jpegs(files[2:3])
    assert sizes1 == sizes[2:3] and torch.equal(det1[0], want_det[2]) and torch.equal(mask1[0], want_mask[2])
    L = _mod("_lib")
    with pytest.raises(L.MrcnnError) as e:
        model.predict_jpegs(files + files[:1])
    assert e.value.code == 4
    with pytest.raises(L.MrcnnError) as e:
        model.predict_jpegs(files[:2] + [data_of("refused")])
    assert e.value.code == ERR_UNSUPPORTED and "file 2 of the batch" in str(e.value)


def test_evaluate_segm_takes_jpeg_bytes(model):
    E, J = _mod("evaluate"), _mod("jpeg")
    names = ["restarts", "odd_422", "grey", "narrow", "custom_tables", "odd_420"]
    as_bytes = [(30 - i, data_of(n)) for i, n in enumerate(names)]
    as_arrays = [(i, J.decode_host(f)) for i, f in as_bytes]
    blob_b, secs_b, recs_b, coco_b = E.evaluate_segm(model, as_bytes, limit=None, verbose=False, batch=4)
    blob_a, secs_a, recs_a, coco_a = E.evaluate_segm(model, as_arrays, limit=None, verbose=False, batch=4)
    assert blob_b == blob_a and len(secs_b) == len(names)
    assert coco_b == coco_a and len(coco_b) > 0
