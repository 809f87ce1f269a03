"""`inference_sliding` of the 3-D model wrappers (pytorchdeeplearing_amd/model/seg_models.py): resample -> normalise -> overlapping windows
through the network -> blended probabilities -> one threshold / arg-max -> back to the source grid -> `postprocess`.  Models are built the
way tests/test_wrappers.py builds them: f32 run dtype, a 16^3 patch, random (perturbed) weights.  The blend restatement and the margin rule
are those of tests/test_sliding_window.py."""
import numpy as np
import pytest
import torch

import conftest
from test_sliding_window import all_entries, check_mask, ref_blend, ref_finalize, ref_window

PATCH = (16, 16, 16)
_models = {}


def _model(dev, monkeypatch, cls, numclass, batch_size=3):
    """one wrapper per (class, device) for the whole module: construction plans the engine, the tests only read it"""
    import model
    from oracle import seg_oracle as seg
    monkeypatch.setenv("SEGENGINE_DTYPE", "f32")
    key = (cls, numclass, dev.type)
    if key not in _models:
        m = getattr(model, cls)(image_depth=16, image_height=16, image_width=16, image_channel=1, numclass=numclass, batch_size=batch_size,
                                use_cuda=dev.type == "cuda")
        kind = "vnet" if "VNet" in cls else "unet"
        m.model.load_state_dict(seg.perturb_params(seg.init_params(kind, 3, 1, numclass, seed=0), seed=7))
        _models[key] = m
    m = _models[key]
    m.postprocess = None
    return m


def _normalised(m, arr):
    """the volume as `inference_sliding` hands it to the window loop when newSpacing == spacing (the linear resample is the identity there)"""
    from pytorchdeeplearing_amd import prepost as pp
    vol = torch.from_numpy(arr).to(m.device)
    return pp.normalize_meanstd(vol, -100.0, 100.0) if m._norm3d == "meanstd" else pp.normalize_percentile(vol)


def _volume(shape, seed):
    return (np.random.RandomState(seed).randn(*shape) * 60.0).astype(np.float32)


@pytest.mark.parametrize("cls,numclass", [("BinaryVNet3dModel", 1), ("MutilUNet3dModel", 3)])
def test_one_window_equals_predict(dev, monkeypatch, cls, numclass):
    """one window of weight 1: acc / wsum is the network's probability itself, so the mask is predict()'s, bit for bit"""
    if cls == "BinaryVNet3dModel":
        conftest.checker_slow(dev, "the host-checker run keeps one wrapper (20-30 s each)")
    m = _model(dev, monkeypatch, cls, numclass)
    arr = _volume(PATCH, 21)
    got = m.inference_sliding(arr, newSpacing=(1.0, 1.0, 1.0), spacing=(1.0, 1.0, 1.0), blend="constant")
    want = m.predict(_normalised(m, arr).cpu().numpy()[None])
    assert got.shape == arr.shape and got.dtype == arr.dtype
    assert np.array_equal(got.astype(np.uint8), want)
    assert 0 < int((want != 0).sum()) < want.size                  # a non-trivial mask
    if numclass == 1:
        assert set(np.unique(got)) <= {0, m._mask_scale}


@pytest.mark.parametrize("cls,numclass", [("BinaryVNet3dModel", 1), ("MutilUNet3dModel", 3)])
def test_multiple_windows_against_the_restatement(dev, monkeypatch, cls, numclass):
    """two windows x an x mirror, gaussian blend: the per-window probabilities come from the same model's own forward, the blend and the
    decision from the fp64 restatement"""
    from pytorchdeeplearing_amd import prepost as pp
    conftest.checker_slow(dev, "eight window forwards take 1-2 min on the host checker")
    m = _model(dev, monkeypatch, cls, numclass)
    shape = (16, 16, 24)
    arr = _volume(shape, 22)
    got, probs = m.inference_sliding(arr, newSpacing=(1.0, 1.0, 1.0), spacing=(1.0, 1.0, 1.0), blend="gaussian", mirror_axes=(2,),
                                     return_probs=True)
    norm = _normalised(m, arr).cpu().numpy()
    entries = all_entries(shape, PATCH, 0.5, (2,))
    assert len(entries) == 4
    windows = np.stack([ref_window(norm, e, PATCH) for e in entries])[:, None]
    m.model.eval()
    with torch.no_grad():
        per_window = m.model(torch.from_numpy(np.ascontiguousarray(windows)).to(m.device))[1].float().cpu().numpy()
    ref_p, ref_mask, margin = ref_finalize(*ref_blend(shape, PATCH, entries, per_window, [pp.importance_1d(p, "gaussian") for p in PATCH]),
                                           scale=m._mask_scale if numclass == 1 else 1)
    assert tuple(probs.shape) == (numclass,) + shape and probs.device.type == m.device.type
    err = np.abs(probs.cpu().numpy() - ref_p).max()
    print("blended probabilities: max |d| = %.2e" % err)
    assert err <= 1e-5
    check_mask(got.astype(np.uint8), ref_mask, margin)
    if numclass > 1:
        # multi-class probabilities: the blend of soft-max outputs still sums to one
        assert np.abs(probs.sum(0).cpu().numpy() - 1.0).max() <= 1e-5


def test_postprocess_hook_sees_the_device_mask_once(dev, monkeypatch):
    m = _model(dev, monkeypatch, "BinaryVNet3dModel", 1)
    arr = _volume(PATCH, 23)
    seen = []

    def hook(mask):
        seen.append((mask.dtype, tuple(mask.shape), mask.device.type, int((mask != 0).sum())))
        return torch.zeros_like(mask)
    m.postprocess = hook
    try:
        out = m.inference_sliding(arr, newSpacing=(1.0, 1.0, 1.0), spacing=(1.0, 1.0, 1.0))
    finally:
        m.postprocess = None
    assert len(seen) == 1 and seen[0][:3] == (torch.uint8, arr.shape, m.device.type)
    assert 0 < seen[0][3] < arr.size                                # the hook saw the network's mask ...
    assert out.shape == arr.shape and not out.any()                 # ... and its answer is what comes back


def test_resampled_grid_and_clip(dev, monkeypatch):
    """newSpacing != spacing: the window loop runs on the resampled grid (probabilities come back on it), the mask on the source grid"""
    from pytorchdeeplearing_amd import prepost as pp
    conftest.checker_slow(dev, "two windows on the resampled grid take ~30 s on the host checker")
    m = _model(dev, monkeypatch, "BinaryVNet3dModel", 1)
    arr = (-1024.0 + 224.0 * np.random.RandomState(24).rand(13, 13, 14)).astype(np.float32)
    got, probs = m.inference_sliding(arr, newSpacing=(0.8, 0.8, 0.8), spacing=(1.0, 1.0, 1.0), clip=(-1024.0, -800.0), return_probs=True)
    size, _ = pp.spacing_resample_size(arr.shape, (0.8,) * 3, (1.0,) * 3)
    assert size == (16, 16, 17) and tuple(probs.shape) == (1,) + size
    assert got.shape == arr.shape and got.dtype == arr.dtype and set(np.unique(got)) <= {0, 255}
    p = probs.cpu().numpy()
    assert np.isfinite(p).all() and p.min() >= 0.0 and p.max() <= 1.0


def test_2d_wrapper_has_no_sliding_inference(dev, monkeypatch):
    import model
    monkeypatch.setenv("SEGENGINE_DTYPE", "f32")
    m = model.BinaryVNet2dModel(image_height=16, image_width=16, image_channel=1, numclass=1, batch_size=1, use_cuda=dev.type == "cuda")
    with pytest.raises(AttributeError):
        m.inference_sliding(np.zeros((16, 16, 16), np.float32))
