"""Network level of the classifiers ResNet3d / ResNet2d (SEG_NET_RESNET): module surface against what the live reference shows (tests/golden/
resnet_modules.json), the plain-torch restatement tests/cls_oracle.py against goldens recorded from the reference (tools/make_golden_cls.py), and the
engine against both - on the host checker and on the GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import cls_oracle
import conftest
from oracle.make_golden import grad_summary, tensor_sha256
from pytorchdeeplearing_amd import _capi, losses, networks
from pytorchdeeplearing_amd.engine import SegEngine

GOLDEN = conftest.GOLDEN
CASE = {c[0]: c for c in cls_oracle.CASES}
TAGS = [c[0] for c in cls_oracle.CASES]
# minutes on the host checker: the 3-D cases (3 min at 16^3, more at 16 x 32 x 48); the 2-D cases (20 s each) keep the planner and the head on the checker
SLOW_ON_CHECKER = ("resnet3d_bin_16", "resnet3d_mc2_v6")
# train steps on the checker: one binary and one multi-class f32 case (1 min each: Adam and the weight re-pack over 2.5 M parameters dominate); the other
# six cases take 1 - 2 min each there and run on the GPU
STEP_ON_CHECKER = (("BinaryCrossEntropyLoss", "f32"), ("MutilFocalLoss", "f32"))


@functools.lru_cache(maxsize=None)
def golden(tag):
    return dict(np.load(os.path.join(GOLDEN, tag + ".npz")))


@functools.lru_cache(maxsize=None)
def modules_record():
    with open(os.path.join(GOLDEN, "resnet_modules.json")) as f:
        return json.load(f)


def module(ndim, in_ch, numclass, dtype="f32"):
    return getattr(networks, "ResNet%dd" % ndim)(in_ch, numclass, dtype=dtype)


@functools.lru_cache(maxsize=None)
def case_data(tag):
    """(params, x, y, eval result, train result, masks, eval result fp64, train result fp64) of a case: the oracle on the CPU, computed once and shared
    (never modified).  The float32 evaluation is what the goldens pin (the reference ran in float32); the engine is compared with the SAME restatement
    evaluated in float64: torch's float32 CPU convolutions are themselves up to 0.9 % off on the gradients of the input block at 16 x 32 x 48 (conv biases in
    front of a GroupNorm with two channels per group: cancelling pairs), depending on the host's CPU and thread count - measured on the GPU host, where the
    engine's f32 gradients agree with the float64 evaluation to 6e-6 on every tensor while the float32 evaluation misses the 5e-3 bound on five of them."""
    _, ndim, shape, numclass, loss, seed = CASE[tag]
    if not torch.cuda.is_available():
        conftest.emu_library()           # (the module reads its parameter table from whichever library serves the host)
    params = cls_oracle.seeded_params(module(ndim, shape[1], numclass), networks.initialize_weights, seed)
    x, y = cls_oracle.batch(shape, numclass)
    G = golden(tag)
    masks = [torch.from_numpy(G["train_masks"][i, :, :c].astype(np.float32)) for i, c in enumerate(G["train_mask_channels"])]
    # one thread, as the generator ran the reference: the `sum` column of a conv weight gradient in front of a GroupNorm is a sum of ~6e5 terms that cancel
    # to rounding noise, and torch's multi-threaded conv backward partitions (and rounds) that noise differently
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ev = cls_oracle.forward_backward(params, x, y, loss)
        tr = cls_oracle.forward_backward(params, x, y, loss, masks=masks)
    finally:
        torch.set_num_threads(nt)
    p64 = {k: v.double() for k, v in params.items()}
    ev64 = cls_oracle.forward_backward(p64, x.double(), y, loss)
    tr64 = cls_oracle.forward_backward(p64, x.double(), y, loss, masks=masks)
    return params, x, y, ev, tr, masks, ev64, tr64


# ------------------------------------------------------------------------------------------------------------------------------------------
# module surface
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_module_tree_matches_live_reference():
    conftest.emu_library()
    recs = modules_record()["tree"]
    assert [(r["cls"], tuple(r["args"])) for r in recs] == [("ResNet3d", (1, 2)), ("ResNet2d", (3, 1))]
    assert [r["numel"] for r in recs] == [7410082, 2554177]
    for rec in recs:
        ours = getattr(networks, rec["cls"])(*rec["args"])
        a = ours.state_dict()
        assert len(a) == 70 and list(a.keys()) == rec["keys"]
        assert [list(v.shape) for v in a.values()] == rec["shapes"]
        assert sum(v.numel() for v in a.values()) == rec["numel"]
        assert [type(m).__name__ for m in ours.modules() if not list(m.children())] == rec["leaves"]
        assert isinstance(ours.fc_layers[0], torch.nn.Linear) and isinstance(ours.fc_layers[2], torch.nn.Linear)
        assert list(a.keys()) == list(cls_oracle.resnet_param_shapes(ours._ndim, *rec["args"]).keys())
        eng = ours.engine
        assert eng.n_drop == 4 and eng.drop_channels == [32, 64, 128, 256] == cls_oracle.dropout_channels() and eng.drop_ld == 256
        assert eng.lib.seg_dropout_calls(eng.h) == 4 and eng.lib.seg_param_count(eng.h) == 70


def test_initialize_weights_draws_the_reference_values():
    conftest.emu_library()
    recs = modules_record()["init"]
    assert [(r["cls"], tuple(r["args"]), r["seed"]) for r in recs] == [("ResNet3d", (1, 2), 110), ("ResNet2d", (1, 3), 111)]
    for rec in recs:
        ours = getattr(networks, rec["cls"])(*rec["args"], dtype="f32")
        torch.manual_seed(rec["seed"])
        ours.apply(networks.initialize_weights)
        a = ours.state_dict()
        assert list(a.keys()) == list(rec["sha256"].keys())
        for k in a:
            assert tensor_sha256(a[k]) == rec["sha256"][k], k
        k = "fc_layers.0.weight"            # the values are in the engine's flat buffer (the views alias it), not in detached copies
        assert tensor_sha256(ours.engine.param_view(k)) == rec["sha256"][k]


def test_unknown_kind_and_bad_shapes_are_refused():
    import ctypes as C
    lib = conftest.emu_library()
    h = C.c_void_p()
    assert lib.seg_create(3, 3, 1, 1, 16, 0, C.byref(h)) < 0
    assert lib.seg_create(_capi.NET_KIND["resnet"], 3, 1, 1, 16, 0, C.byref(h)) == 0
    assert lib.seg_plan(h, 1, 16, 16, 24) < 0            # not a multiple of 16
    lib.seg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------------
# oracle against the reference goldens (CPU)
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_vs_golden(tag):
    """tests/cls_oracle.py against what the reference computed; the tolerances of tests/test_oracle.py::test_net_restatement_vs_golden"""
    params, x, y, ev, tr, masks, _, _ = case_data(tag)
    G = golden(tag)
    assert abs(float(x.double().sum()) - float(G["x_sum"])) < 1e-9 and np.array_equal(y.numpy(), G["y"])
    assert list(G["train_mask_channels"]) == cls_oracle.dropout_channels()
    names = list(G["grad_names"])
    for r, pre, gk in ((ev, "eval", "grad_summary"), (tr, "train", "train_grad_summary")):
        np.testing.assert_allclose(r["logits"].numpy(), G[pre + "_logits"], rtol=0, atol=2e-5)
        assert abs(float(r["loss"]) - float(G[pre + "_loss"])) < 1e-6
        assert names == list(r["grads"].keys())
        np.testing.assert_allclose(np.stack([grad_summary(r["grads"][k]) for k in names]), G[gk], rtol=2e-3, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------------------------------------
# engine against oracle and golden
# ------------------------------------------------------------------------------------------------------------------------------------------
def engine_step(e, x, y, loss, mask_mode, masks=None):
    """forward -> loss -> backward through the separate library calls; (logits, probs, loss, grads)"""
    logits, probs = e.forward(x, mask_mode, masks)
    out3 = e.loss_forward(logits, y, loss, class_alpha=None)
    dl = e.loss_backward(logits, y, loss)
    e.backward(dl, zero_grads=True)
    return logits.cpu(), probs.cpu(), float(out3[0]), {k: v.cpu().clone() for k, v in e.grad_dict().items()}


def check_grads(got, ref):
    for k, r in ref.items():
        r = r.double()
        assert float((got[k].double() - r).norm()) <= 5e-3 * float(r.norm()) + 1e-9, (k, float((got[k] - r).norm()), float(r.norm()))


@pytest.mark.parametrize("tag", TAGS)
def test_engine_vs_oracle_and_golden(dev, tag):
    """f32 run dtype: eval logits within 1e-4 of oracle and golden, loss within 1e-5, every parameter gradient ||d|| <= 5e-3 ||ref|| + 1e-9; the same for a
    train-mode step with the multipliers the reference drew (SEG_MASKS_GIVEN).
    The oracle is evaluated in float64 (see case_data); the goldens are the reference's float32 run."""
    if tag in SLOW_ON_CHECKER:
        conftest.checker_slow(dev)
    _, ndim, shape, numclass, loss, _ = CASE[tag]
    params, x, y, _, _, masks, ev, tr = case_data(tag)
    G = golden(tag)
    e = SegEngine("resnet", ndim, shape[1], numclass, dtype="f32", device=dev)
    e.load_state_dict(params)
    xd, yd = x.to(dev), y.to(dev)
    logits, probs, lv, grads = engine_step(e, xd, yd, loss, _capi.MASKS_EVAL)
    assert tuple(logits.shape) == (shape[0], numclass) == tuple(probs.shape)
    assert float((logits - ev["logits"]).abs().max()) < 1e-4 and float((logits - torch.from_numpy(G["eval_logits"])).abs().max()) < 1e-4
    p = torch.sigmoid(logits) if numclass == 1 else torch.softmax(logits, 1)
    assert float((probs - p).abs().max()) < 1e-6
    assert abs(lv - float(ev["loss"])) < 1e-5 and abs(lv - float(G["eval_loss"])) < 1e-5
    check_grads(grads, ev["grads"])
    # train-mode step with the multipliers the reference drew
    logits, probs, lv, grads = engine_step(e, xd, yd, loss, _capi.MASKS_GIVEN, masks)
    assert float((logits - torch.from_numpy(G["train_logits"])).abs().max()) < 1e-4 and float((logits - tr["logits"]).abs().max()) < 1e-4
    assert abs(lv - float(G["train_loss"])) < 1e-5
    check_grads(grads, tr["grads"])
    names = list(G["grad_names"])
    gs = np.stack([grad_summary(grads[k]) for k in names])
    ref = G["train_grad_summary"]
    assert np.all(np.abs(gs[:, 1] - ref[:, 1]) <= 5e-3 * ref[:, 1] + 1e-9)             # the norms the reference recorded
    # the finished gradients form a suffix that starts with the four FC tensors: after the first two backward ops (fill, head) they are final
    k, off, nops = e.backward_bucket(1e-9)
    assert (k, off) == (2, e.table["fc_layers.0.weight"][1]) and nops > 2
    prev = e.numel
    for frac in (0.01, 0.3, 0.6, 1.0):
        k, off, _ = e.backward_bucket(frac)
        assert off <= prev and e.numel - off >= frac * e.numel - 1
        prev = off


LOSS_CASES = [("BinaryCrossEntropyLoss", 1), ("BinaryFocalLoss", 1), ("MutilCrossEntropyLoss", 3), ("MutilFocalLoss", 3)]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("loss,numclass", LOSS_CASES)
def test_train_step_lowers_the_loss(dev, loss, numclass, dtype):
    """five one-call steps (seg_train_step: forward, loss with v = 1, backward, Adam) on a fixed batch, dropout off so that the curve is a function of the
    step alone"""
    if (loss, dtype) not in STEP_ON_CHECKER:
        conftest.checker_slow(dev, "five train steps take 1 - 2 min on the host checker")
    e = SegEngine("resnet", 2, 1, numclass, dtype=dtype, device=dev)
    torch.manual_seed(3)
    net = module(2, 1, numclass)
    net.apply(networks.initialize_weights)
    e.load_state_dict(net.state_dict())
    x, y = cls_oracle.batch((2, 1, 16, 16), numclass, seed=4)          # the smallest plan: level 4 is one pixel
    x, y = x.to(dev), y.to(dev)
    alpha = torch.ones(numclass, device=dev) if numclass > 1 else None
    curve = [float(e.train_step(x, y, loss, lr=1e-3, weight_decay=0.0, decoupled=False, class_alpha=alpha, mask_mode=_capi.MASKS_EVAL)[0]) for _ in range(5)]
    print(loss, dtype, curve)
    assert all(np.isfinite(curve)) and curve[-1] < curve[0], curve
    assert int(e.opt_state[0]) == 5 and e.skipped_steps == 0


def test_reference_style_use(dev):
    """loss module -> backward -> torch optimiser acting on the parameter views; state_dict round trip; train() draws masks in the engine"""
    torch.manual_seed(0)
    net = module(2, 1, 1)
    net.apply(networks.initialize_weights)
    net = net.to(dev)
    x, y = cls_oracle.batch((2, 1, 32, 32), 1, seed=2)
    x, y = x.to(dev), y.to(dev)
    net.eval()
    logits = net(x)
    assert torch.is_tensor(logits) and tuple(logits.shape) == (2, 1)
    ref = cls_oracle.forward_backward({k: v.detach().cpu().double() for k, v in net.state_dict().items()}, x.cpu().double(), y.cpu(), "BinaryCrossEntropyLoss")
    assert float((logits.detach().cpu() - ref["logits"]).abs().max()) < 1e-4
    opt = torch.optim.Adam(net.parameters())
    loss = losses.BinaryCrossEntropyLoss()(logits, y)
    opt.zero_grad()
    loss.backward()
    assert abs(float(loss.detach()) - float(ref["loss"])) < 1e-5
    check_grads({k: p.grad.cpu() for k, p in net.named_parameters()}, ref["grads"])
    before = net.engine.params.clone()
    opt.step()
    assert not torch.equal(before, net.engine.params)        # the optimiser wrote straight into the flat buffer
    net2 = module(2, 1, 1).to(dev)
    net2.load_state_dict(net.state_dict())
    net2.eval()
    l1, l2, l3 = net(x), net2(x), net(x)
    assert torch.equal(l1, l2) and torch.equal(l1, l3)       # eval is reproducible, and a round trip through state_dict changes nothing
    lg, pr = net.forward_probs(x)
    assert torch.equal(lg, l1) and float((pr - torch.sigmoid(lg)).abs().max()) < 1e-6
    net.train()
    t1, t2 = net(x), net(x)
    assert not torch.equal(t1, l1) and not torch.equal(t1, t2)


@pytest.mark.gpu
def test_graph_replay_equals_stream_launches():
    """the captured step of a classifier replays the launches of the stream path (the gates of tests/test_engine.py::test_graph_replay_equals_stream_launches:
    the same loss curve and parameters up to the run-to-run noise of the GroupNorm statistics' atomics)"""
    dev = torch.device("cuda:0")
    _capi.product_library()
    params, x, y = case_data("resnet3d_bin_16")[:3]
    xd, yd = x.to(dev), y.to(dev)
    runs = {}
    for mode in ("stream", "graph"):
        e = SegEngine("resnet", 3, 1, 1, dtype="f16", device=dev)
        e.load_state_dict(params)
        logits = torch.empty((2, 1), dtype=torch.float32, device=dev)
        probs = torch.empty_like(logits)
        curve = [float(e.train_step(xd, yd, "BinaryCrossEntropyLoss", lr=1e-3, logits=logits, probs=probs, launch=mode)[0]) for _ in range(5)]
        torch.cuda.synchronize()
        assert e.lib.seg_train_graph_ready(e.h) == (1 if mode == "graph" else 0), getattr(e, "graph_error", None)
        assert int(e.opt_state[0]) == 5 and int(e.lib.seg_dropout_draws(e.h)) == 5
        runs[mode] = (curve, e.params.detach().cpu().clone())
        del e
    (c0, p0), (c1, p1) = runs["stream"], runs["graph"]
    assert max(abs(a - b) for a, b in zip(c0, c1)) < 2e-3, (c0, c1)
    d = (p0 - p1).abs()
    assert float(d.max()) <= 5 * 1e-3 + 1e-6 and float((d > 1e-4).float().mean()) < 0.2
