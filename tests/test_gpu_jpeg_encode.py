"""JPEG encode on the GPU (mrcnn_jpeg_encode_batch; kernels_jpeg_enc.hip): colour conversion, downsampling, forward DCT, quantisation,
Huffman coding and byte stuffing in a fixed number of launches for a ragged batch.  The expectation is the scalar definition
mrcnn_jpeg_encode_host — itself held to libjpeg in tests/test_jpeg_encode_host.py — and every comparison is byte for byte."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_enc_v1.npz"))
NAMES = sorted(k[:-7] for k in GOLD.files if k.endswith("_pixels"))
SENTINEL = 0xA5
ERR_SHAPE = 4


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def case(name):
    quality, sampling = (int(v) for v in GOLD[name + "_params"])
    return np.ascontiguousarray(GOLD[name + "_pixels"]), quality, sampling


@pytest.fixture(scope="module")
def big():
    """One 120x200 image (15 x 25 blocks of luma: the scans span several chunks, the launches several thread blocks) and the
    definition's file for each sampling mode, computed once."""
    yy, xx = np.mgrid[0:120, 0:200]
    rng = np.random.default_rng(11)
    img = np.stack([(xx * 3 + yy) % 256, (yy * 2 + xx // 2 + 60) % 256, ((xx + yy) * 2) % 256], -1) + rng.integers(-30, 31, (120, 200, 3))
    img = np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8))
    return img, {s: _mod("jpeg").encode_host(img, 90, s) for s in range(4)}


def raw_call(images, quality, sampling, capacity, device=False, misalign=0, null_out=False):
    """One mrcnn_jpeg_encode_batch into a sentinel-filled buffer of `capacity` + 64 bytes → (status, buffer, offsets).  device: the
    pixels are uploaded first, all into one tensor, each image `misalign` bytes past a 16-byte boundary."""
    L = _mod("_lib")
    B = len(images)
    table = (L.Image * B)()
    keep = []
    if device:
        import torch
        starts, total = [], 0
        for im in images:
            starts.append(total + misalign)
            total += (im.size + misalign + 15) // 16 * 16
        dev = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        for b, im in enumerate(images):
            dev[starts[b]:starts[b] + im.size] = torch.from_numpy(im.reshape(-1)).cuda()
            table[b].rgb, table[b].height, table[b].width = dev.data_ptr() + starts[b], im.shape[0], im.shape[1]
        torch.cuda.synchronize()
        keep.append(dev)
    else:
        for b, im in enumerate(images):
            table[b].rgb, table[b].height, table[b].width = im.ctypes.data, im.shape[0], im.shape[1]
    out = np.full(capacity + 64, SENTINEL, np.uint8)
    offs = np.full(B + 1, -1, np.int64)
    st = L.lib().mrcnn_jpeg_encode_batch(table, B, L.DEVICE if device else L.HOST, quality, sampling, None if null_out else out.ctypes.data, capacity,
                                         offs.ctypes.data)
    del keep
    return st, out, offs


@pytest.mark.parametrize("where", ["host", "device", "device+1"])
@pytest.mark.parametrize("name", NAMES)
def test_each_case_alone_equals_the_definition(name, where):
    pixels, quality, sampling = case(name)
    want = _mod("jpeg").encode_host(pixels, quality, sampling)
    st, out, offs = raw_call([pixels], quality, sampling, len(want), device=where != "host", misalign=1 if where == "device+1" else 0)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    assert offs.tolist() == [0, len(want)]
    got = out[:len(want)].tobytes()
    assert got == want, f"{name}: first difference at byte {next(i for i in range(len(want)) if got[i] != want[i])} of {len(want)}"
    assert (out[len(want):] == SENTINEL).all()                      # nothing behind file_offsets[batch] is touched


@pytest.mark.parametrize("where", ["host", "device+1"])
@pytest.mark.parametrize("sampling", [0, 1, 2, 3])
def test_all_cases_as_one_ragged_batch(sampling, where):
    """Every fixture image in one call (the call takes one quality and one sampling: each mode in turn, at the quality of the mode's
    own fixture cases), files back to back."""
    jpeg = _mod("jpeg")
    quality = {0: 90, 1: 75, 2: 75, 3: 75}[sampling]
    images = [case(n)[0] for n in NAMES]
    want = [jpeg.encode_host(im, quality, sampling) for im in images]
    total = sum(len(w) for w in want)
    st, out, offs = raw_call(images, quality, sampling, total, device=where != "host", misalign=1)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for b, n in enumerate(NAMES):
        assert out[offs[b]:offs[b + 1]].tobytes() == want[b], f"file {b} ({n})"
    assert (out[total:] == SENTINEL).all()


@pytest.mark.parametrize("sampling", [0, 1, 2, 3])
def test_a_larger_image_equals_the_definition(big, sampling):
    img, want = big
    files = _mod("jpeg").encode_batch([img], 90, sampling)
    assert len(files) == 1 and len(files[0]) > 4 * 128               # several chunks of scan
    assert files[0] == want[sampling]


def test_more_blocks_than_one_round_of_the_scan():
    """The one-block scan of the bit counts covers 4096 blocks a round: 33 x 125 = 4125 grey blocks take two, and the image behind
    them starts where their carry says."""
    jpeg = _mod("jpeg")
    yy, xx = np.mgrid[0:264, 0:1000]
    g = ((xx * 5 + yy * 7) % 256 + np.random.default_rng(4).integers(-20, 21, (264, 1000))).clip(0, 255).astype(np.uint8)
    images = [np.ascontiguousarray(np.stack([g] * 3, -1)), case("odd_420")[0]]
    files = jpeg.encode_batch(images, 75, "grey")
    assert files == [jpeg.encode_host(im, 75, "grey") for im in images]


def test_capacity_protocol(big):
    img, want = big
    images = [img, case("odd_420")[0]]
    files = [want[2], _mod("jpeg").encode_host(images[1], 90, 2)]
    total = len(files[0]) + len(files[1])
    st, out, offs = raw_call(images, 90, 2, 0, null_out=True)         # the size query
    assert st == 0 and offs.tolist() == [0, len(files[0]), total]
    st, out, offs = raw_call(images, 90, 2, total - 1)                # one byte short: an error naming the capacity, nothing written
    assert st == ERR_SHAPE and str(total) in _mod("_lib").lib().mrcnn_last_error().decode()
    assert offs.tolist() == [0, len(files[0]), total] and (out == SENTINEL).all()
    st, out, offs = raw_call(images, 90, 2, total + 32, device=True)  # a larger buffer: the bytes written are the size reported
    assert st == 0 and offs[2] == total and out[:total].tobytes() == files[0] + files[1] and (out[total:] == SENTINEL).all()


def test_round_trip_on_the_device_equals_the_hosts(big):
    jpeg = _mod("jpeg")
    img, want = big
    images = [img] + [case(n)[0] for n in ("odd_420", "one_pixel", "even_420")]
    files = jpeg.encode_batch(images, 90, "420")
    decoded, sizes = jpeg.decode_batch(files, device=True)
    assert sizes == [im.shape[:2] for im in images]
    for b, im in enumerate(images):
        np.testing.assert_array_equal(decoded[b].cpu().numpy(), jpeg.decode_host(jpeg.encode_host(im, 90, "420")), err_msg=f"image {b}")


def test_render_jpegs_decodes_to_the_rendered_images(small_model):
    import torch
    jpeg, models = _mod("jpeg"), _mod("models")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype="f32x3")
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(96, 160), (37, 53)]]
    rendered = m.render_images(images)
    want = [jpeg.decode_host(jpeg.encode_host(r, 90, "420")) for r in rendered]
    for source in (images, [torch.from_numpy(im).cuda() for im in images]):      # numpy in, and device tensors in (the overlay stays there)
        files = m.render_jpegs(source)
        assert len(files) == 2 and all(isinstance(f, bytes) for f in files)
        for b in range(2):
            np.testing.assert_array_equal(jpeg.decode_host(files[b]), want[b], err_msg=f"image {b}")
    files = m.render_jpegs(images, quality=50, sampling="444", alpha=256, stroke=0, min_score=0.0)      # keyword arguments reach both halves
    opaque = m.render_images(images, alpha=256, stroke=0, min_score=0.0)
    for b in range(2):
        assert files[b] == jpeg.encode_host(opaque[b], 50, "444")


def test_the_plain_c_host_writes_the_mirrors_file(small_model, tmp_path):
    import subprocess
    from test_c_host import _build_example
    exe = _build_example(tmp_path, "maskrcnn_render_jpeg")
    d, cfg = small_model
    img = np.random.default_rng(21).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    (tmp_path / "img.rgb").write_bytes(img.tobytes())
    env = {k: v for k, v in os.environ.items() if k != "MRCNN_TEST_KNOBS"}     # a production process
    r = subprocess.run([exe, d, str(tmp_path / "img.rgb"), "100", "150", str(tmp_path / "out.jpg")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "out.jpg").read_bytes()
    assert r.stdout.split()[2:] == ["bytes", str(len(blob))] and int(r.stdout.split()[1]) > 0
    m = _mod("models").load_maskrcnn(d, max_batch=1)                            # the mirror names no precision either
    assert blob == m.render_jpegs([img])[0]
    assert _mod("jpeg").info(blob)["height"] == 100 and _mod("jpeg").info(blob)["width"] == 150
