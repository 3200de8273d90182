"""The float64 stage-wise reference (oracle/network.py: stem64, stage64, fpn64, rpn64, classifier64, mask64) on CPU.

The stages chained must be the graph the fp32 oracle network evaluates (same layer list, strides, upsampling, P6) — checked against
that network's own code evaluated in float64 with the same float32 BN fold — and the torch-CPU fp32 network must sit within the
fp32 figure of profiles/r06_fp64_trunk_parity.json (torch_cpu_fp32: 3.7e-6) of them.  round_f16 leaves fp16 values unchanged.
"""
import numpy as np
import pytest
import torch

from conftest import rand_images


@pytest.fixture(scope="module")
def small(small_model):
    from oracle.network import load_oracle_model
    d, cfg = small_model
    return load_oracle_model(d), cfg, rand_images(2, cfg.image_height, cfg.image_width, seed=4)


def _chain(om, images, f16=False):
    c = [om.stem64(images, f16)]
    for st in (2, 3, 4, 5):
        c.append(om.stage64(st, c[-1], f16))
    p = om.fpn64(c[1:], f16)
    return c, p, om.rpn64(p, f16)


def test_chained_stages_equal_the_graph_in_float64(small):
    from oracle import network as N
    om, cfg, images = small
    c, p, (probs, deltas) = _chain(om, images)
    pyr, tp, td = om.trunk_fp64(images)
    assert all(np.array_equal(a, b) for a, b in zip(p, pyr)) and np.array_equal(probs, tp) and np.array_equal(deltas, td)
    # the graph code of the fp32 network (backbone / fpn / rpn), in float64 with the engine's fold
    w32 = om.w
    om.w = N._W({k: v.numpy() for k, v in w32.t.items()}, torch.float64, folded=True)
    try:
        with torch.no_grad():
            feats = om.backbone(om.preprocess(images).to(torch.float64))
            gp = om.fpn(feats)
            gprobs, gdeltas = om.rpn(gp)
    finally:
        om.w = w32
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for a, b in zip(c[1:], feats):
        assert a.shape == b.shape and rel(a, b.numpy()) <= 1e-12
    for a, b in zip(p, gp[:4]):
        assert a.shape == b.shape and rel(a, b.numpy()) <= 1e-12
    assert rel(probs, gprobs.numpy()) <= 1e-12 and rel(deltas, gdeltas.numpy()) <= 1e-12
    assert c[0].shape == (2, 64, cfg.image_height // 4, cfg.image_width // 4)


def test_torch_fp32_network_within_the_r06_fp32_figure(small):
    from oracle.network import channel_error
    om, cfg, images = small
    c, p, (probs, deltas) = _chain(om, images)
    pyr, oprobs, odeltas = om.trunk(images)
    for a, ref in zip(pyr, p):
        assert channel_error(a, ref) < 4e-6
    assert np.abs(oprobs - probs).max() < 4e-6 and channel_error(odeltas, deltas, axis=2) < 4e-6
    # the heads on the float64 P's samples: same network code in fp32 against float64
    rng = np.random.default_rng(2)
    pooled = np.maximum(rng.standard_normal((5, 256, cfg.classifier_pool_size, cfg.classifier_pool_size)), 0).astype(np.float32)
    op, ob = om.classifier_model(pooled)
    rp, rb = om.classifier64(pooled)
    assert np.abs(op - rp).max() < 4e-6 and channel_error(ob, rb) < 4e-6
    pm = np.maximum(rng.standard_normal((3, 256, cfg.mask_pool_size, cfg.mask_pool_size)), 0).astype(np.float32)
    assert np.abs(om.mask_model(pm) - om.mask64(pm)).max() < 4e-6


def test_round_f16_is_idempotent_on_fp16_input(small):
    from oracle.network import round_to_f16
    om, cfg, images = small
    x = np.random.default_rng(3).standard_normal((1000,)).astype(np.float16).astype(np.float64)
    assert np.array_equal(round_to_f16(x), x)
    assert np.array_equal(round_to_f16(torch.from_numpy(x)).numpy(), x)
    # every stage's output with round_f16 is fp16-exact (its last operation is an fp16 store), and the stage is a function of it
    c, p, _ = _chain(om, images, f16=True)
    for t in c + p:
        assert np.array_equal(round_to_f16(t), t)
    assert np.array_equal(om.stage64(3, round_to_f16(c[1]), True), c[2])
    assert not np.array_equal(c[2], om.stage64(3, c[1], False))          # the option changes the evaluation
    pooled = round_to_f16(np.maximum(np.random.default_rng(4).standard_normal((2, 256, 7, 7)), 0))
    a, b = om.classifier64(pooled, True), om.classifier64(pooled, False)
    assert np.abs(a[0] - b[0]).max() > 0
