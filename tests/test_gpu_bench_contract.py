"""bench.py's output contract, on a reduced workload so it runs in seconds: exactly one JSON line on stdout carrying the
driver's fields plus, under --full, the `roofline` and `cpu_baseline` objects (and `other_modes`), also through torch.distributed.run
with the RCCL leg forced at world size 1; a plain run carries the driver's fields alone and dumps its outputs on request."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ["--arch", "resnet50", "--size", "256", "--batch", "2", "--steps", "3", "--warmup", "1"]
SMALL = ["--full", "--cpu-images", "1", "--e2e-images", "2"] + PLAIN


def _check(line, n_gpus=1, steps=3, warmup=1):
    j = json.loads(line)
    for k, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                   ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(j[k], typ), k
    assert j["metric"].startswith("images/sec") and j["unit"] == "images/s" and j["higher_is_better"] is True
    assert j["n_gpus"] == n_gpus and j["steps"] == steps and j["warmup"] == warmup and j["scaling"] == "weak"
    assert j["vs_baseline"] is None and j["data"] == "synthetic" and "workload" in j["config"] and "model" not in j["config"]
    assert abs(j["value"] - n_gpus * 2 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-2            # whole-job images per second
    r = j["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r and r["kernel"].startswith(("k_conv_", "k_bneck_"))
    # round 5: the backbone subset (north_star's target is worded on it) and the same-run box normaliser
    b = r["backbone_convs"]
    assert 0 < b["frac"] < 1 and b["launches_per_step"] > 0 and 0 < b["share_of_step_time"] < r["all_conv_kernels"]["share_of_step_time"]
    live = r["sustained_peak_live"]
    assert live["unit"] == "TFLOP/s" and live["value"] > 0 and 0 < r["frac_of_live_sustained"] < 1.2
    assert abs(r["frac_of_live_sustained"] - r["achieved"] / live["value"]) < 2e-3
    # round 6: every tile class says which roof bounds it and carries both rates; the instrumented steps are their own, behind the timed region
    assert r["instrumented"]["steps"] >= 1 and r["instrumented"]["ms_per_step"] > 0
    for name, c in r["by_tile_class"].items():
        assert c["bound"] in ("hbm", "mfma"), name
        assert c["algorithmic_bytes_per_launch"] > 0 and c["gbps"] > 0 and 0 < c["frac_of_hbm"] < 1.5 and 0 < c["frac_of_mfma"] < 1, (name, c)
        assert abs(c["frac_of_hbm"] - c["gbps"] / 8000.0) < 1e-3 and c["launches_per_step"] >= 1
    assert sum(c["share_of_step_time"] for c in r["by_tile_class"].values()) == pytest.approx(r["all_conv_kernels"]["share_of_step_time"], abs=2e-3)
    assert "model_loaded_by" in j["config"]
    return j


def test_bench_json_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                                   # ONE line on stdout
    j = _check(lines[0])
    c = j["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["unit"] == "images/s" and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert c["value"] < j["value"]
    assert c["images"] == 1 and c["ms_per_image"]["min"] <= c["ms_per_image"]["median"] <= c["ms_per_image"]["max"]
    # the model was loaded WITHOUT naming a precision (MRCNN_DEFAULT) from an artefact calibrated the way `convert --calibrate` does: -> f32x3
    assert j["dtype"] == "f32x3" and r_peak(j) == pytest.approx(2500.0 / 3, rel=1e-3)
    assert j["config"]["model_loaded_by"].startswith("MRCNN_DEFAULT") and "stored split exponents" in j["config"]["model_loaded_by"]
    assert j["split"]["source"].startswith("stored in MaskRCNN.mrcw")
    assert set(j["other_modes"]) == {"f32", "f32s", "f16"} and all(v["value"] > 0 for v in j["other_modes"].values())
    assert all(v["steps"] >= 10 for v in j["other_modes"].values())
    assert all(0 < v["roofline"]["backbone_convs"]["frac"] < 1 and 0 < v["roofline"]["all_conv_kernels"]["frac"] < 1 for v in j["other_modes"].values())
    g = j["gpu_busy"]
    assert 0 < g["gpu_seconds"] <= g["wall_seconds"] * 1.001 and g["predicts"] == j["steps"]       # measured in this run
    # (round 6: neither leg carries events any more.  On this reduced workload — ~200 launches for a few hundred microseconds of GPU work — a
    #  step is bound by the HOST's enqueue, and the pipelined entry keeps two batches in flight where the resident loop synchronises every
    #  step: the host-buffer rate may legitimately come out above the resident one here; at the headline size the two agree within 2 %)
    assert j["h2d_included"]["value"] > 0 and j["h2d_included"]["value"] <= j["value"] * 1.6
    assert "not measured in this run" in j["profiles_ref"]["note"].lower()
    p = j["parity_e2e"]
    assert p["images"] == 2 and set(p["modes"]) == {"f32", "f32x3", "f32s", "f16"}
    assert p["modes"]["f32x3"]["fraction"] >= 0.9 and p["modes"]["f32"]["fraction"] >= 0.9


def r_peak(j):
    return j["roofline"]["peak"]


def test_bench_gpus_1_without_torchrun_prints_n_gpus_1():
    """The driver's N = 1 command line (`python bench.py --gpus 1 ...`, no torchrun) stays a single-process run."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-other-modes"] + SMALL,
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = _check(lines[0])
    assert j["config"]["parallelism"] == "single"


def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) is set-up, warm-up, the timed steps and the line: the driver's fields, none of the --full records.
    --dump-outputs writes what the last timed step handed its caller, and two runs of the same arguments write the same arrays."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(d)] + PLAIN,
                           capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout
        j = json.loads(lines[0])
        assert j["metric"].startswith("images/sec") and j["unit"] == "images/s" and j["higher_is_better"] is True and j["dtype"] == "f32x3"
        assert j["steps"] == 3 and j["warmup"] == 1 and j["gpu_busy"]["predicts"] == 3                # exactly --steps timed steps
        assert abs(j["value"] - 2 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-2
        for k in ("roofline", "stage_ms_last_step", "profiles_ref", "other_modes", "h2d_included", "cpu_baseline", "parity_e2e"):
            assert k not in j, k
        assert sorted(os.listdir(d)) == ["detections.npy", "masks.npy"]
        det, mask = np.load(d / "detections.npy"), np.load(d / "masks.npy")
        assert det.dtype == mask.dtype == np.float32 and det.shape[0] == mask.shape[0] == 2 and det.shape[2] == 6
        assert mask.shape[1] == det.shape[1] and int((det[0, :, 5] > 0).sum()) == j["config"]["detections_image0"] > 0
        dumps.append((det, mask))
    np.testing.assert_array_equal(dumps[0][0], dumps[1][0])
    np.testing.assert_array_equal(dumps[0][1], dumps[1][1])


def test_bench_self_launch_covers_the_visible_gpus():
    """`python bench.py --gpus N` with no torchrun environment launches its N ranks itself: with N GPUs an N-rank line
    (parallelism dpN), otherwise a loud failure — never n_gpus: 1."""
    import torch
    n = 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--no-cpu-baseline", "--no-other-modes"] + SMALL,
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    if torch.cuda.device_count() >= n:
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
        assert len(lines) == 1
        j = _check(lines[0], n_gpus=n)
        assert j["config"]["parallelism"] == f"dp{n}"
    else:
        assert r.returncode != 0 and not r.stdout.strip() and f"--gpus {n}" in r.stderr


def test_bench_under_torchrun_with_rccl_leg():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--no-cpu-baseline",
           "--no-other-modes"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                                   # RCCL's banner must not reach stdout
    j = _check(lines[0])
    assert "cpu_baseline" not in j and "other_modes" not in j
    # the N > 1 path stays warm on one GPU: the native exchange ran, on the RCCL copy the process already holds
    assert j["rccl"]["native_shares_process_copy"] == 1
    pr = j["per_rank_ms_per_step"]
    assert len(pr["ranks"]) == 1 and pr["min"] == pr["max"] == pr["ranks"][0] and abs(pr["max"] - j["ms_per_step"]) < 1e-6


def test_mfma_probe_and_profile_groups_behind_the_test_header():
    """The two measurement entries bench.py's round-5 fields rest on: the in-process MFMA probe (plausible rates for both matrix
    instructions, clock equivalent inside the part's range) and the backbone / other split of the conv profile (every launch in exactly
    one group; the backbone's algorithmic work per image = conv1 + res2..res5 of the architecture)."""
    import ctypes as C
    import importlib
    import tempfile
    import numpy as np
    L = importlib.import_module("mask-rcnn-coreml_amd._lib")
    tf, mhz = C.c_double(0), C.c_double(0)
    L.check(L.lib().mrcnn_bench_mfma_probe(0.3, L.F16, C.byref(tf), C.byref(mhz)))
    assert 800 < tf.value < 2600 and 800 < mhz.value < 2600, (tf.value, mhz.value)
    L.check(L.lib().mrcnn_bench_mfma_probe(0.3, L.F32, C.byref(tf), C.byref(mhz)))
    assert 80 < tf.value < 160 and 1200 < mhz.value < 2600, (tf.value, mhz.value)
    with pytest.raises(L.MrcnnError):
        L.check(L.lib().mrcnn_bench_mfma_probe(0.3, L.F32S, C.byref(tf), None))
    pkg = importlib.import_module("mask-rcnn-coreml_amd")
    models = importlib.import_module("mask-rcnn-coreml_amd.models")
    weights = importlib.import_module("mask-rcnn-coreml_amd.weights")
    cfg = pkg.ModelConfig(architecture="resnet50", input_image_shape=(256, 256, 3), num_classes=21, pre_nms_max_proposals=500, max_proposals=64, max_detections=16)
    d = tempfile.mkdtemp(prefix="mrcnn_grp_")
    weights.save_synthetic_models(d, cfg, seed=0, forced_load=True)
    for mode in ("f32x3", "f16"):
        m = models.load_maskrcnn(d, max_batch=2, compute_dtype=mode)
        img = np.random.default_rng(0).integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
        m.predict(img)
        m.conv_profile_enable(True)
        m.predict(img)
        m.conv_profile_enable(False)
        tiles, groups = m.conv_profile(), m.conv_profile_groups()
        assert sum(v[0] for v in tiles.values()) == groups["backbone"][0] + groups["other"][0] > 0
        assert abs(sum(v[2] for v in tiles.values()) - groups["backbone"][2] - groups["other"][2]) < 1e-6 * groups["other"][2]
        # ResNet-50 backbone C1..C5 at 1024^2: 4.93 + 27.92 + 39.73 + 57.98 + 30.60 = 161.16 GFLOP per image (SURVEY 8d's per-stage figures;
        # BASELINE.md section 2's 189.8 adds the box head's 28.62 by mistake); at 256^2 a sixteenth of it
        per_image = groups["backbone"][2] / 2 / 1e9
        assert abs(per_image - 161.16 / 16) < 0.005 * 161.16 / 16, per_image
        # round 6: ALGORITHMIC bytes ride with every launch (what the hbm roofs of bench.py's by_tile_class are priced against): the per-class and
        # per-shape totals agree, and one layer by hand — the FPN's 3x3 output layer on P2 (2 images x 64 x 64 pixels, 256 -> 256): its input
        # pixels once, its fp16 filters, its output
        by_tile, shapes = m.conv_profile_bytes(), m.conv_profile_shapes()
        assert sum(by_tile.values()) > 0 and abs(sum(by_tile.values()) - sum(r[7] for r in shapes)) < 1e-6 * sum(by_tile.values())
        es = 2 if mode == "f16" else 4
        p2 = [r for r in shapes if (r[0], r[1], r[2]) == (2 * 64 * 64, 256, 2304)]
        assert len(p2) == 1 and p2[0][4] == 1, p2
        assert p2[0][7] == 2 * 64 * 64 * 256 * es + 256 * 2304 * 2 + 2 * 64 * 64 * 256 * es, p2
        del m
