"""PNG encode on the GPU (mrcnn_png_encode_batch; kernels_png.hip): the raw stream regenerated from the samples, the token bits
counted per deflate block and scanned, every token ORed into the files, Adler-32 from per-block sums, in a fixed number of launches
for a ragged batch.  The expectation is the sequential definition mrcnn_png_encode_host — itself held to an independent restatement
in tests/test_png_host.py — and every comparison is byte for byte."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "png_v1.npz"))
NAMES = sorted(k[:-7] for k in GOLD.files if k.endswith("_pixels"))
SENTINEL = 0xA5
ERR_SHAPE = 4


def _mod(name):
    return importlib.import_module("mask-rcnn-coreml_amd." + name)


def case(name):
    pixels = np.ascontiguousarray(GOLD[name + "_pixels"])
    return pixels, int(GOLD[name + "_rows"])


def fmt_of(pixels):
    return 1 if pixels.dtype == np.int16 else 0


def first_difference(got, want):
    return next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))


def raw_call(images, rows, capacity, device=False, misalign=0, null_out=False):
    """One mrcnn_png_encode_batch into a sentinel-filled buffer of `capacity` + 64 bytes → (status, buffer, offsets).  device: the
    pixels are uploaded first, all into one tensor, each image `misalign` bytes past a 16-byte boundary."""
    L = _mod("_lib")
    B = len(images)
    table = (L.PngSource * B)()
    keep = []
    if device:
        import torch
        starts, total = [], 0
        for im in images:
            starts.append(total + misalign)
            total += (im.nbytes + misalign + 15) // 16 * 16
        dev = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        for b, im in enumerate(images):
            dev[starts[b]:starts[b] + im.nbytes] = torch.from_numpy(im.reshape(-1).view(np.uint8)).cuda()
            table[b].pixels, table[b].height, table[b].width = dev.data_ptr() + starts[b], im.shape[0], im.shape[1]
        torch.cuda.synchronize()
        keep.append(dev)
    else:
        for b, im in enumerate(images):
            table[b].pixels, table[b].height, table[b].width = im.ctypes.data, im.shape[0], im.shape[1]
    out = np.full(capacity + 64, SENTINEL, np.uint8)
    offs = np.full(B + 1, -1, np.int64)
    st = L.lib().mrcnn_png_encode_batch(table, B, L.DEVICE if device else L.HOST, fmt_of(images[0]), rows, None if null_out else out.ctypes.data, capacity,
                                        offs.ctypes.data)
    del keep
    return st, out, offs


@pytest.mark.parametrize("where", ["host", "device", "device+misaligned"])
@pytest.mark.parametrize("name", NAMES)
def test_each_case_alone_equals_the_definition(name, where):
    pixels, rows = case(name)
    want = _mod("png").encode_host(pixels, rows or None)
    assert want == GOLD[name + "_file"].tobytes()                    # (the definition is the fixture's: tests/test_png_host.py)
    st, out, offs = raw_call([pixels], rows, len(want), device=where != "host", misalign=pixels.itemsize if where == "device+misaligned" else 0)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    assert offs.tolist() == [0, len(want)]
    got = out[:len(want)].tobytes()
    assert got == want, f"{name}: first difference at byte {first_difference(got, want)} of {len(want)}"
    assert (out[len(want):] == SENTINEL).all()                      # nothing behind file_offsets[batch] is touched


@pytest.mark.parametrize("where", ["host", "device+misaligned"])
@pytest.mark.parametrize("kind", ["grey", "instance"])
def test_all_cases_of_a_format_as_one_ragged_batch(kind, where):
    """Every fixture image of a format in one call, files back to back: they start at odd byte offsets, so the tokens of one file
    share words with the frame of the file before.  (The call takes one `rows`: the instance cases are both written at 255.)"""
    png = _mod("png")
    images = [case(n)[0] for n in NAMES if (case(n)[0].dtype == np.int16) == (kind == "instance")]
    rows = 255 if kind == "instance" else 0
    want = [png.encode_host(im, rows or None) for im in images]
    assert any(int(o) % 4 for o in np.cumsum([len(w) for w in want])[:-1])
    total = sum(len(w) for w in want)
    st, out, offs = raw_call(images, rows, total, device=where != "host", misalign=images[0].itemsize)
    assert st == 0, _mod("_lib").lib().mrcnn_last_error()
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    for b, w in enumerate(want):
        got = out[offs[b]:offs[b + 1]].tobytes()
        assert got == w, f"file {b}: first difference at byte {first_difference(got, w)} of {len(w)}"
    assert (out[total:] == SENTINEL).all()


def test_more_blocks_than_one_round_of_the_scan():
    """The one-block scan of the bit counts covers 4096 deflate blocks a round: 2049 x 8191 zeros are 2049 * 8192 / 4096 = 4098 blocks
    and take two, and the image behind them starts where their carry says.  Every block but the first starts inside a run."""
    png = _mod("png")
    images = [np.zeros((2049, 8191), np.uint8), case("random")[0]]
    files = png.encode_batch(images)
    want = [png.encode_host(im) for im in images]
    assert [len(f) for f in files] == [len(w) for w in want]
    assert files == want


def test_capacity_protocol():
    png = _mod("png")
    images = [case("instance_255")[0], case("instance_1")[0]]
    files = [png.encode_host(im, 255) for im in images]
    total = len(files[0]) + len(files[1])
    st, out, offs = raw_call(images, 255, 0, null_out=True)           # the size query
    assert st == 0 and offs.tolist() == [0, len(files[0]), total]
    st, out, offs = raw_call(images, 255, total - 1)                  # one byte short: an error naming the capacity, nothing written
    assert st == ERR_SHAPE and str(total) in _mod("_lib").lib().mrcnn_last_error().decode()
    assert offs.tolist() == [0, len(files[0]), total] and (out == SENTINEL).all()
    st, out, offs = raw_call(images, 255, total + 32, device=True)    # a larger buffer: the bytes written are the size reported
    assert st == 0 and offs[2] == total and out[:total].tobytes() == files[0] + files[1] and (out[total:] == SENTINEL).all()


def test_the_chain_from_detections_to_files_stays_on_the_device():
    """Synthetic detections and 28x28 masks → detection.instance_map_source on CUDA tensors → png.encode_batch on the maps where they
    lie: the file's index - 1 is the map, and the file is the definition's for the map copied back."""
    import torch
    from test_gpu_render import MODEL_H, MODEL_W, ROWS, _synthetic
    png, D = _mod("png"), _mod("detection")
    sizes = [(37, 427), (250, 333), (2, 5), (7, 1), (96, 150)]
    det, masks = _synthetic(sizes)
    _, maps, _ = D.instance_map_source(torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), sizes, MODEL_H, MODEL_W, 0.5, 0.0)
    assert all(m.is_cuda and m.dtype == torch.int16 for m in maps)
    files = png.encode_batch(maps, rows=ROWS)
    assert sum(int((m >= 0).sum()) for m in maps) > 1000             # (something was drawn)
    for b, m in enumerate(maps):
        host = m.cpu().numpy()
        parsed = png.parse(files[b])
        assert all(ok for _, _, ok in parsed["chunks"]) and parsed["colour_type"] == 3 and len(parsed["palette"]) == ROWS + 1
        np.testing.assert_array_equal(parsed["scanlines"].astype(np.int16) - 1, host, err_msg=f"image {b}")
        assert files[b] == png.encode_host(host, ROWS), f"image {b}"


def test_mask_planes_leave_as_grey_files():
    """The uint8 planes of detection.paste_masks_source, a file per plane in one call (what MRCNN_PNG_MAX_BATCH = 1024 is for)."""
    import torch
    from test_gpu_render import MODEL_H, MODEL_W, ROWS, _synthetic
    png, D = _mod("png"), _mod("detection")
    sizes = [(37, 53), (20, 31)]
    det, masks = _synthetic(sizes)
    _, planes = D.paste_masks_source(det, masks, sizes, MODEL_H, MODEL_W, 0.5)
    assert sum(int(p.sum()) for p in planes) > 1000                  # (something was pasted)
    on_device = [torch.from_numpy(p).cuda() for p in planes]
    flat = [on_device[b][i] for b in range(len(sizes)) for i in range(ROWS)]
    files = png.encode_batch(flat)
    assert len(files) == len(sizes) * ROWS
    for k, f in enumerate(files):
        assert f == png.encode_host(planes[k // ROWS][k % ROWS]), f"plane {k}"


def test_instance_pngs_parse_back_to_the_maps(small_model):
    import torch
    png, models, D = _mod("png"), _mod("models"), _mod("detection")
    d, cfg = small_model
    m = models.load_maskrcnn(d, max_batch=2, compute_dtype="f32x3")
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(96, 160), (37, 53)]]
    det, mask = m.predict_images(images)
    _, want, _ = D.instance_map_source(det, mask, [im.shape[:2] for im in images], m.image_height, m.image_width)
    for source in (images, [torch.from_numpy(im).cuda() for im in images]):      # numpy in, and device tensors in (the maps stay there)
        files = m.instance_pngs(source)
        assert len(files) == 2 and all(isinstance(f, bytes) for f in files)
        for b in range(2):
            parsed = png.parse(files[b])
            assert len(parsed["palette"]) == m.max_detections + 1
            np.testing.assert_array_equal(parsed["scanlines"].astype(np.int16) - 1, want[b], err_msg=f"image {b}")
    files = m.instance_pngs(images, min_score=0.5, threshold=0.6)                 # keyword arguments reach the map
    _, cut, _ = D.instance_map_source(det, mask, [im.shape[:2] for im in images], m.image_height, m.image_width, threshold=0.6, min_score=0.5)
    for b in range(2):
        assert files[b] == png.encode_host(cut[b], m.max_detections)


def test_the_plain_c_host_writes_the_mirrors_file(small_model, tmp_path):
    import subprocess
    from test_c_host import _build_example
    exe = _build_example(tmp_path, "maskrcnn_instance_png")
    d, cfg = small_model
    img = np.random.default_rng(21).integers(0, 256, (100, 150, 3), dtype=np.uint8)
    (tmp_path / "img.rgb").write_bytes(img.tobytes())
    env = {k: v for k, v in os.environ.items() if k != "MRCNN_TEST_KNOBS"}     # a production process
    r = subprocess.run([exe, d, str(tmp_path / "img.rgb"), "100", "150", str(tmp_path / "out.png")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    blob = (tmp_path / "out.png").read_bytes()
    assert r.stdout.split()[2:] == ["bytes", str(len(blob))] and int(r.stdout.split()[1]) >= 0
    m = _mod("models").load_maskrcnn(d, max_batch=1)                            # the mirror names no precision either
    assert blob == m.instance_pngs([img])[0]
    parsed = _mod("png").parse(blob)
    assert (parsed["height"], parsed["width"]) == (100, 150) and all(ok for _, _, ok in parsed["chunks"])
