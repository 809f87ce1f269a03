"""CPU checks of the Grad-CAM yardsticks: the plain-torch restatement tests/gradcam_oracle.py against the maps recorded from the reference's own GradCAM
class (tests/golden/gradcam_2d.npz, tools/make_golden_gradcam.py), and against the live class where the reference tree is present."""
import functools
import os

import numpy as np
import pytest
import torch

import conftest
import gradcam_oracle as gco
from oracle import ref_loader

CASE = {c[0]: c for c in gco.CASES_2D}
KEYS = [(c[0], ls, k) for c in gco.CASES_2D for ls in gco.LAYER_SETS for k in gco.golden_classes(c[3])]


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(conftest.GOLDEN, "gradcam_2d.npz")))


@functools.lru_cache(maxsize=None)
def oracle_feats(tag, cls, dtype=torch.float32):
    params, x = gco.case_inputs(tag)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)             # as the generator ran the reference
    try:
        return gco.features(params, x, cls, dtype=dtype)[1]
    finally:
        torch.set_num_threads(nt)


def test_fixture_lists_what_the_tool_writes():
    G = golden()
    assert list(G["layer_sets"]) == list(gco.LAYER_SETS) and list(G["cases"]) == [c[0] for c in gco.CASES_2D]
    assert sorted(k for k in G if k not in ("layer_sets", "cases")) == sorted(k + s for t, ls, c in KEYS for k in [gco.golden_key(t, ls, c)] for s in ("", "_raw"))
    assert os.path.getsize(os.path.join(conftest.GOLDEN, "gradcam_2d.npz")) < 324 * 1024


@pytest.mark.parametrize("tag,layer_set,cls", KEYS)
def test_restatement_vs_golden(tag, layer_set, cls):
    """the oracle in float32 against what the reference's class computed: atol 2e-5, the bound test_resnet.py::test_restatement_vs_golden uses for the
    logits (the float32 : float64 spread of the maps was measured at 2.7e-6); the raw maps' extrema to 1e-6 + 1e-4 relative"""
    G = golden()
    names = gco.LAYER_SETS[layer_set]
    feats = oracle_feats(tag, cls)
    shape = CASE[tag][2]
    got = gco.cam_map(feats, names, shape[2:]).float().numpy()
    ref = G[gco.golden_key(tag, layer_set, cls)]
    assert got.shape == ref.shape == (shape[0],) + tuple(shape[2:]) and ref.dtype == np.float32
    print(tag, layer_set, cls, "max |d|", float(np.abs(got - ref).max()))
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5)
    assert float(ref.min()) >= 0.0 and float(ref.max()) <= 1.0
    raw = G[gco.golden_key(tag, layer_set, cls) + "_raw"]
    assert raw.shape == (len(names), shape[0], 2)
    for i, n in enumerate(names):
        r = gco.raw_map(*feats[n]).reshape(shape[0], -1)
        np.testing.assert_allclose(torch.stack([r.min(1).values, r.max(1).values], 1).float().numpy(), raw[i], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("cls", [1, 2])
def test_all_negative_maps_are_exactly_zero(cls):
    """resnet2d_mc3_32, down_tr256, classes 1 and 2: the raw map is negative everywhere (by 50 x the 16-bit rounding), the reference returns zeros.
    A check of the yardstick: class 2 is also held against the recorded map; the fixture holds no class 1 (first and last class only), so that case tests the
    restatement alone and passes with or without the feature - the engine's side is tests/test_gradcam_engine.py::test_all_negative_maps_are_exactly_zero."""
    feats = oracle_feats("resnet2d_mc3_32", cls)
    raw = gco.raw_map(*feats["down_tr256"])
    assert float(raw.max()) < -0.04
    m = gco.cam_map(feats, ("down_tr256",), (32, 32))
    assert torch.count_nonzero(m) == 0 and not torch.isnan(m).any()
    if cls == 2:
        G = golden()
        assert np.count_nonzero(G["resnet2d_mc3_32__down_tr256__c2"]) == 0 and float(G["resnet2d_mc3_32__down_tr256__c2_raw"][..., 1].max()) < -0.04


@pytest.mark.skipif(not ref_loader.available(), reason="reference tree only exists in the build container")
def test_restatement_and_golden_vs_live_reference():
    """the reference's class itself: it reproduces a recorded map, and the restatement follows it on a layer set and class the fixture does not hold.
    Both at the float32 bound of test_restatement_vs_golden: torch's float32 convolutions round differently with the thread count (the fixture was
    recorded with one thread), which alone moves map values by 1.3e-6"""
    nets, GradCAM = gco.load_reference_gradcam()
    case = CASE["resnet2d_mc3_32"]
    live, raw = gco.reference_maps(nets, GradCAM, case, ("down_tr256",), 0)
    G = golden()
    np.testing.assert_allclose(live, G["resnet2d_mc3_32__down_tr256__c0"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(raw, G["resnet2d_mc3_32__down_tr256__c0_raw"], rtol=1e-4, atol=1e-6)
    names = ("down_tr32", "down_tr128")
    live, _ = gco.reference_maps(nets, GradCAM, case, names, 1)
    got = gco.cam_map(oracle_feats("resnet2d_mc3_32", 1), names, (32, 32)).float().numpy()
    print("max |d|", float(np.abs(got - live).max()))
    np.testing.assert_allclose(got, live, rtol=0, atol=2e-5)
