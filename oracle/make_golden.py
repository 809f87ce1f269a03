"""TEST INFRASTRUCTURE ONLY.  Regenerate tests/golden/*.npz by running the REAL reference
(/root/reference, imported via oracle.ref_loader) on seeded synthetic inputs in the build container.

    python -m oracle.make_golden

The fixtures pin oracle/seg_oracle.py (and through it the HIP engine) to the reference's actual
outputs; /root/reference itself does not exist on the GPU box.  Sizes are tiny so the files stay
small (a few hundred KB in total)."""
import os
import sys

import numpy as np
import torch

from . import ref_loader

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def _np(t):
    return t.detach().cpu().numpy()


def make_losses(nets, losses, metric):
    # SURVEY.md §8(c) recipe — order of draws matters
    torch.manual_seed(0)
    z = torch.randn(2, 1, 8, 8, 8)
    y = (torch.rand(2, 8, 8, 8) > 0.7).long()
    z4 = torch.randn(2, 4, 8, 8, 8)
    y4 = torch.randint(0, 4, (2, 8, 8, 8))
    a = torch.ones(4)
    out = dict(z=_np(z), y=_np(y), z4=_np(z4), y4=_np(y4))
    for name, f, args in (
            ("BinaryDiceLoss", losses.BinaryDiceLoss(), (z, y)),
            ("BinaryCrossEntropyLoss", losses.BinaryCrossEntropyLoss(), (z, y)),
            ("BinaryFocalLoss", losses.BinaryFocalLoss(), (z, y)),
            ("BinaryCrossEntropyDiceLoss", losses.BinaryCrossEntropyDiceLoss(), (z, y)),
            ("MutilDiceLoss", losses.MutilDiceLoss(a), (z4, y4)),
            ("MutilCrossEntropyLoss", losses.MutilCrossEntropyLoss(a), (z4, y4)),
            ("MutilFocalLoss_g2", losses.MutilFocalLoss(a, gamma=2), (z4, y4)),
            ("MutilFocalLoss_g3", losses.MutilFocalLoss(a, gamma=3), (z4, y4))):
        zz = args[0].clone().requires_grad_(True)
        val = f(zz, args[1])
        val.backward()
        out["loss_" + name] = _np(val)
        out["grad_" + name] = _np(zz.grad)
    out["dice_coeff"] = _np(metric.dice_coeff(torch.sigmoid(z), y))
    out["iou_coeff"] = _np(metric.iou_coeff(torch.sigmoid(z), y))
    out["multiclass_dice_coeff"] = _np(metric.multiclass_dice_coeff(torch.softmax(z4, 1), y4))
    np.savez_compressed(os.path.join(OUT, "losses_metrics.npz"), **out)
    print("losses:", {k: float(v) for k, v in out.items() if k.startswith("loss_")})


def make_losses_extra(losses):
    """the model/losses.py classes no wrapper selects but which the engine implements from the same sums"""
    torch.manual_seed(0)
    z = torch.randn(2, 1, 8, 8, 8)
    y = (torch.rand(2, 8, 8, 8) > 0.7).long()
    z4 = torch.randn(2, 4, 8, 8, 8)
    y4 = torch.randint(0, 4, (2, 8, 8, 8))
    y4[y4 == 3] = 2                                   # class 3 absent: exercises the present-class mask
    a = torch.tensor([0.5, 1.0, 1.5, 1.0])
    out = dict(z=_np(z), y=_np(y), z4=_np(z4), y4=_np(y4), alpha=_np(a))
    for name, f, args in (
            ("BinaryJaccardLoss", losses.BinaryJaccardLoss(), (z, y)),
            ("BinaryELDiceLoss", losses.BinaryELDiceLoss(), (z, y)),
            ("BinaryTverskyLoss", losses.BinaryTverskyLoss(), (z, y)),
            ("BinarySSLoss", losses.BinarySSLoss(), (z, y)),
            ("MutilCrossEntropyDiceLoss", losses.MutilCrossEntropyDiceLoss(a), (z4, y4)),
            ("MutilELDiceLoss", losses.MutilELDiceLoss(a), (z4, y4))):
        zz = args[0].clone().requires_grad_(True)
        val = f(zz, args[1])
        val.backward()
        out["loss_" + name] = _np(val)
        out["grad_" + name] = _np(zz.grad)
    # ---- multi-label use of the binary classes: [N, C > 1, ...] logits with a same-shaped 0/1 target (model/losses.py:43-53 `view(bs, num_classes, -1)`)
    zml = torch.randn(2, 3, 6, 6, 6)
    yml = (torch.rand(2, 3, 6, 6, 6) > 0.6).float()
    out["zml"], out["yml"] = _np(zml), _np(yml)
    for name, f in (("BinaryDiceLoss", losses.BinaryDiceLoss()), ("BinaryCrossEntropyDiceLoss", losses.BinaryCrossEntropyDiceLoss()),
                    ("BinaryFocalLoss", losses.BinaryFocalLoss()), ("BinaryTverskyLoss", losses.BinaryTverskyLoss()),
                    ("BinarySSLoss", losses.BinarySSLoss()), ("BinaryJaccardLoss", losses.BinaryJaccardLoss())):
        zz = zml.clone().requires_grad_(True)
        val = f(zz, yml)
        val.backward()
        out["mlloss_" + name] = _np(val)
        out["mlgrad_" + name] = _np(zz.grad)
    # ---- the rest of model/losses.py (round 3).  LOSS_REPAIRS: what a user of the reference has to do before these classes run at all
    tv = losses.MutilTverskyLoss(a); tv.beta = 0.7
    ss = losses.MutilSSLoss(a); ss.r = 0.1
    p = torch.sigmoid(z)
    lov_z = torch.randn(2, 8, 8, 8)                  # BinaryLovaszLoss takes [B, ...] logits and labels of the same shape
    out["lov_z"] = _np(lov_z)
    for name, f, args in (
            ("MutilTverskyLoss", tv, (z4, y4)),
            ("MutilSSLoss", ss, (z4, y4)),
            ("MCC_Loss", losses.MCC_Loss(), (p, y.unsqueeze(1).float())),
            ("BinaryLovaszLoss", losses.BinaryLovaszLoss().forward, (lov_z, y)),
            ("LovaszLoss", losses.LovaszLoss(), (z4, y4))):
        zz = args[0].clone().requires_grad_(True)
        val = f(zz, args[1])
        val.backward()
        out["loss_" + name] = _np(val)
        out["grad_" + name] = _np(zz.grad)
    np.savez_compressed(os.path.join(OUT, "losses_extra.npz"), **out)
    print("extra losses:", {k: float(v) for k, v in out.items() if k.startswith("loss_")})


LOSS_REPAIRS = (
    ("MutilTverskyLoss", "instance attribute beta = 0.7", "losses.py:449 reads self.beta, which __init__ (:431-434) never sets; 0.7 is BinaryTverskyLoss's value (:111)"),
    ("MutilSSLoss", "instance attribute r = 0.1", "losses.py:413 reads self.r, which __init__ (:395-398) never sets; 0.1 is BinarySSLoss's value (:84)"),
    ("BinaryLovaszLoss", "called through .forward()", "losses.py:237 calls super(BinaryLovaszLoss).__init__() (unbound super): nn.Module.__init__ never runs, "
                                                      "so __call__ fails on the missing hook tables; forward() itself runs as written"),
    ("MCC_Loss", "none", "losses.py:224-227 use the torch 1.x overload torch.add(input, alpha, other) = input + alpha*other, still accepted (deprecated) by torch 2.10"),
    ("LovaszLoss", "none", "losses.py:473 hands the logits to _lovasz_softmax as `probas`; no soft-max is applied - reproduced as written"),
)


METRIC_REPAIRS = (
    # model/metric.py:210 — `assert input.size() == target.size()` can never hold next to the F.one_hot of index labels two
    # lines above it (one-hot needs (N, V) indices, the assert needs (N, C, V)); with it removed the function body runs as written
    ("    assert input.size() == target.size()\n", "", "metric.py:210: unsatisfiable size assert"),
)


def make_ssim():
    """model/lossesSSIM.py run as shipped: SSIM (2-D, size_average True / False) and SSIM3D on small volumes, values and gradients
    with respect to both images."""
    import sys as _sys
    ref_loader.load()
    S = _sys.modules["ref_model.lossesSSIM"]
    torch.manual_seed(3)
    a2, b2 = torch.rand(2, 3, 20, 24), torch.rand(2, 3, 20, 24)
    a3 = torch.rand(2, 1, 12, 14, 16)
    b3 = (a3 + 0.2 * torch.randn(2, 1, 12, 14, 16)).clamp(0, 1)
    out = dict(a2=_np(a2), b2=_np(b2), a3=_np(a3), b3=_np(b3))
    for tag, f, (x, y) in (("ssim2d", S.SSIM(window_size=11, size_average=True), (a2, b2)),
                           ("ssim2d_w7", lambda p, q: S.ssim(p, q, window_size=7), (a2, b2)),
                           ("ssim3d", S.SSIM3D(window_size=11), (a3, b3))):
        xx, yy = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        v = f(xx, yy)
        v.backward()
        out["val_" + tag], out["g1_" + tag], out["g2_" + tag] = _np(v), _np(xx.grad), _np(yy.grad)
    xx = a2.clone().requires_grad_(True)
    v = S.SSIM(window_size=11, size_average=False)(xx, b2)
    (v * torch.tensor([1.0, -2.0])).sum().backward()
    out["val_ssim2d_persample"], out["g1_ssim2d_persample"] = _np(v), _np(xx.grad)
    # ssim3D(size_average=False): `.mean(1).mean(1).mean(1)` of the 5-D map leaves (N, W) (model/lossesSSIM.py:92-97)
    xx, yy = a3.clone().requires_grad_(True), b3.clone().requires_grad_(True)
    v = S.ssim3D(xx, yy, window_size=11, size_average=False)
    wts = torch.linspace(-1.0, 2.0, v.numel()).reshape(v.shape)
    (v * wts).sum().backward()
    out["val_ssim3d_cols"], out["w_ssim3d_cols"], out["g1_ssim3d_cols"], out["g2_ssim3d_cols"] = _np(v), _np(wts), _np(xx.grad), _np(yy.grad)
    np.savez_compressed(os.path.join(OUT, "ssim.npz"), **out)
    print("ssim:", {k: np.asarray(v).tolist() for k, v in out.items() if k.startswith("val_")})


def make_metric_extra(metric):
    """M4 multiclass_iou_coeff (model/metric.py:204-215): the reference's own function text with METRIC_REPAIRS applied in
    memory, on the section-8(c) recipe inputs (+ a case with an absent class)."""
    import re
    src = open(os.path.join(ref_loader.REF, "model", "metric.py")).read()
    m = re.search(r"^def multiclass_iou_coeff\(.*?(?=^def |\Z)", src, re.S | re.M)
    text = m.group(0)
    for old, new, _why in METRIC_REPAIRS:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    ns = {"torch": torch, "F": torch.nn.functional, "Tensor": torch.Tensor, "iou_coeff": metric.iou_coeff}
    exec(compile(text, "metric_repaired", "exec"), ns)
    torch.manual_seed(0)
    _z = torch.randn(2, 1, 8, 8, 8)
    _y = (torch.rand(2, 8, 8, 8) > 0.7).long()
    z4 = torch.randn(2, 4, 8, 8, 8) * 3.0              # sharper soft-max: a good share of voxels passes the 0.5 threshold
    y4 = torch.randint(0, 4, (2, 8, 8, 8))
    y4b = y4.clone(); y4b[y4b == 3] = 1
    z3 = torch.randn(3, 3, 6, 10) * 3.0
    y3 = torch.randint(0, 3, (3, 6, 10))
    out = dict(z4=_np(z4), y4=_np(y4), y4b=_np(y4b), z3=_np(z3), y3=_np(y3))
    out["miou_a"] = _np(ns["multiclass_iou_coeff"](torch.softmax(z4, 1), y4))
    out["miou_b"] = _np(ns["multiclass_iou_coeff"](torch.softmax(z4, 1), y4b))
    out["miou_2d"] = _np(ns["multiclass_iou_coeff"](torch.softmax(z3, 1), y3))
    out["mdice_a"] = _np(metric.multiclass_dice_coeff(torch.softmax(z4, 1), y4))
    np.savez_compressed(os.path.join(OUT, "metric_extra.npz"), **out)
    print("metric extra:", {k: float(v) for k, v in out.items() if k.startswith("m")})


def grad_summary(g):
    """Compact, order-sensitive fingerprint of one gradient tensor: sum, L2 norm, and 16 entries
    at fixed pseudo-random flat positions."""
    f = g.detach().double().reshape(-1)
    idx = (torch.arange(16, dtype=torch.int64) * 2654435761 + 12345) % f.numel()
    return np.concatenate([[float(f.sum()), float(f.norm())], f[idx].numpy()])


def make_net(nets, losses, seg, tag, kind, ndim, ctor, shape, numclass, loss_mod):
    """eval-mode fwd+bwd (dropout off) and a train-mode fwd with the recorded dropout masks.
    Weights come from oracle.seg_oracle.init_params/perturb_params (seeded, reproducible on the GPU
    box) and are loaded into the REAL reference module with load_state_dict, so only outputs and
    gradient fingerprints need to be stored."""
    m = ctor()
    params = seg.perturb_params(seg.init_params(kind, ndim, shape[1], numclass, seed=0), seed=7)
    missing = m.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    x, y = seg.synthetic_batch(shape[0], shape[2:], shape[1], numclass, seed=1)
    out = dict(x_sum=np.float64(x.double().sum()), y_sum=np.int64(y.sum()))
    m.eval()
    logits, probs = m(x)
    loss = loss_mod(logits, y)
    m.zero_grad()
    loss.backward()
    out["eval_logits"], out["eval_loss"] = _np(logits), _np(loss)
    out["eval_probs_sum"] = np.float64(probs.double().sum())
    names = [k for k, _ in m.named_parameters()]
    out["grad_names"] = np.array(names)
    out["grad_summary"] = np.stack([grad_summary(p.grad) for _, p in m.named_parameters()])
    # train mode: record per-call dropout multipliers (peek the CPU generator before each call)
    masks = []

    def pre(mod, inp):
        xin = inp[0]
        n, c = xin.shape[:2]
        state = torch.get_rng_state()
        mk = torch.empty((n, c) + (1,) * (xin.dim() - 2)).bernoulli_(0.8).div_(0.8)
        torch.set_rng_state(state)           # peek only: the module then consumes the same draws
        masks.append(mk.reshape(n, c).clone())

    hs = [mod.register_forward_pre_hook(pre) for mod in m.modules()
          if isinstance(mod, (torch.nn.Dropout3d, torch.nn.Dropout2d))]
    m.train()
    torch.manual_seed(99)
    logits_t, _ = m(x)
    loss_t = loss_mod(logits_t, y)
    m.zero_grad()
    loss_t.backward()
    for h in hs:
        h.remove()
    out["train_logits"], out["train_loss"] = _np(logits_t), _np(loss_t)
    out["train_grad_summary"] = np.stack([grad_summary(p.grad) for _, p in m.named_parameters()])
    out["train_masks"] = np.stack([np.pad(_np(k), ((0, 0), (0, 256 - k.shape[1]))) for k in masks]).astype(np.float16)
    out["train_mask_channels"] = np.array([k.shape[1] for k in masks])
    np.savez_compressed(os.path.join(OUT, tag + ".npz"), **out)
    print(tag, "logits.sum", float(logits.sum()), "loss", float(loss), "train loss", float(loss_t), "n_masks", len(masks))


CLDICE_REPAIRS = (
    # (reference text, repaired text, why) - applied IN MEMORY to model/lossescldice.py; nothing is written back
    ("shape = x.size().tolist()", "shape = x.dim()", "lossescldice.py:10-11,16: rank test; torch.Size has no tolist()"),
    ("def __int__(self):", "def __init__(self):", "lossescldice.py:43: constructor never ran"),
    ("def __int__(self, alpha):", "def __init__(self, alpha):\n        super(Mutil_Soft_cldice_loss, self).__init__()",
     "lossescldice.py:67: constructor never ran / nn.Module not initialised"),
    ("y_true = y_true.view(input.size())", "y_true = y_true.reshape(input.size()).to(input.dtype)",
     "lossescldice.py:80: permuted view + max_pool on a Long tensor"),
)


def load_repaired_cldice():
    src = open(os.path.join(ref_loader.REF, "model", "lossescldice.py")).read()
    for old, new, _why in CLDICE_REPAIRS:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    ns = {}
    exec(compile(src, "lossescldice_repaired", "exec"), ns)
    return ns


def cldice_inputs(shape, seed, numclass=0):
    """vessel-like probabilities: low-pass noise through a sigmoid; target = another field thresholded."""
    g = torch.Generator().manual_seed(seed)
    nd = len(shape) - 2
    pool = torch.nn.functional.avg_pool3d if nd == 3 else torch.nn.functional.avg_pool2d
    def field(ch):
        t = torch.randn((shape[0], ch) + tuple(shape[2:]), generator=g)
        return pool(pool(t, 3, 1, 1), 3, 1, 1) * 6.0
    if numclass:
        pred = torch.softmax(field(numclass), 1)
        target = field(numclass).argmax(1)
    else:
        pred = torch.sigmoid(field(shape[1]))
        target = (field(shape[1]) > 0.3).float()
    return pred, target


def make_cldice():
    ns = load_repaired_cldice()
    out = {}
    for tag, shape in (("b3", (2, 1, 12, 14, 16)), ("b2", (2, 2, 24, 20))):
        pred, target = cldice_inputs(shape, 77 + len(shape))
        pred.requires_grad_(True)
        out[tag + "_pred"], out[tag + "_target"] = _np(pred), _np(target)
        out[tag + "_skel_pred"] = _np(ns["soft_skeletonize"](pred))
        out[tag + "_skel_target"] = _np(ns["soft_skeletonize"](target))
        loss = ns["Binary_Soft_cldice_loss"]()(pred, target)
        loss.backward()
        out[tag + "_loss"], out[tag + "_dpred"] = _np(loss), _np(pred.grad)
        print("cldice", tag, float(loss))
    for tag, shape, c in (("m3", (1, 3, 8, 10, 12), 3), ("m2", (2, 3, 16, 16), 3)):
        pred, target = cldice_inputs(shape, 91 + len(shape), c)
        pred.requires_grad_(True)
        alpha = torch.tensor([0.5, 1.0, 2.0])
        loss = ns["Mutil_Soft_cldice_loss"](alpha)(pred, target)
        loss.backward()
        out[tag + "_pred"], out[tag + "_target"], out[tag + "_alpha"] = _np(pred), _np(target), _np(alpha)
        out[tag + "_loss"], out[tag + "_dpred"] = _np(loss), _np(pred.grad)
        print("cldice", tag, float(loss))
    np.savez_compressed(os.path.join(OUT, "cldice.npz"), **out)


def load_reference_function(relpath, name, ns):
    """exec ONE top-level function of a reference file (its module cannot be imported here: SimpleITK / cv2 are absent);
    the text is taken verbatim, nothing is written back."""
    import re
    src = open(os.path.join(ref_loader.REF, relpath)).read()
    m = re.search(r"^def %s\(.*?(?=^def |\Z)" % name, src, re.S | re.M)
    assert m, name
    exec(compile(m.group(0), relpath + ":" + name, "exec"), ns)
    return ns[name]


def prepost_inputs():
    """CT-like float32 volumes: smooth noise in Hounsfield-like units, a zero background slab, a constant case."""
    rs = np.random.RandomState(5)
    a = (rs.randn(20, 24, 28) * 300.0).astype(np.float32)
    a[:, :6, :] = 0.0                                        # exact zeros: the "non-zero" statistics differ from the global ones
    b = np.round(rs.randn(9, 11, 13) * 50.0).astype(np.float32)      # integer-valued (int16 CT read as float): many ties
    c = np.full((4, 5, 6), 7.0, np.float32)                  # constant: early return
    d = np.zeros((6, 6, 6), np.float32); d[2:4, 2:4, 2:4] = 3.0      # > 95 % zeros: t == b == 0
    e = rs.rand(17, 3, 5).astype(np.float32) + 1.0           # no zeros at all
    return dict(a=a, b=b, c=c, d=d, e=e)


def make_prepost():
    normalize = load_reference_function(os.path.join("dataprocess", "utils.py"), "normalize", {"np": np})
    out = {}
    import warnings
    for k, v in prepost_inputs().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = normalize(v.copy())
        out["normalize_in_" + k], out["normalize_out_" + k] = v, np.asarray(r)
        print("prepost normalize", k, r.dtype, float(np.asarray(r).mean()))
    np.savez_compressed(os.path.join(OUT, "prepost.npz"), **out)


REF_MODULES = (("VNet3d", (1, 1)), ("UNet3d", (1, 4)), ("VNet2d", (1, 2)), ("UNet2d", (3, 1)))        # module tree
REF_INITS = (("VNet3d", (1, 1)), ("UNet3d", (1, 4)), ("VNet2d", (3, 2)), ("UNet2d", (1, 1)))          # initialize_weights, seed 100 + index
REF_SKIPPED_LEAVES = ("ReLU", "Dropout3d", "Dropout2d", "MaxPool3d", "MaxPool2d")                     # parameter-free leaves the engine folds away


def tensor_sha256(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().float().contiguous().numpy().tobytes()).hexdigest()


def make_reference_modules(nets):
    """the reference networks' state_dict layout, leaf module order and seeded `initialize_weights` values (as SHA-256 of the float32 bytes
    of each tensor) -> tests/golden/reference_modules.json"""
    import json
    out = {"tree": [], "init": []}
    for cls, args in REF_MODULES:
        m = getattr(nets, cls)(*args)
        sd = m.state_dict()
        out["tree"].append({"cls": cls, "args": list(args), "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()],
                            "leaves": [type(x).__name__ for x in m.modules() if not list(x.children()) and type(x).__name__ not in REF_SKIPPED_LEAVES]})
    for seed, (cls, args) in enumerate(REF_INITS):
        m = getattr(nets, cls)(*args)
        torch.manual_seed(100 + seed)
        m.apply(nets.initialize_weights)
        out["init"].append({"cls": cls, "args": list(args), "seed": 100 + seed,
                            "sha256": {k: tensor_sha256(v) for k, v in m.state_dict().items()}})
    with open(os.path.join(OUT, "reference_modules.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("reference modules:", [(t["cls"], len(t["keys"])) for t in out["tree"]])


def main():
    if not ref_loader.available():
        sys.exit("reference tree not available; golden fixtures can only be regenerated in the build container")
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)
    if "--only-reference-modules" in sys.argv:
        make_reference_modules(ref_loader.load()[0])
        return
    if "--only-metric-extra" in sys.argv:
        _nets, _losses, metric = ref_loader.load()
        make_metric_extra(metric)
        return
    if "--only-ssim" in sys.argv:
        make_ssim()
        return
    if "--only-losses-extra" in sys.argv:
        _nets, losses, _metric = ref_loader.load()
        make_losses_extra(losses)
        return
    make_prepost()
    if "--only-prepost" in sys.argv:
        return
    make_cldice()
    if "--only-cldice" in sys.argv:
        return
    nets, losses, metric = ref_loader.load()
    torch.set_num_threads(1)
    make_losses(nets, losses, metric)
    make_losses_extra(losses)
    make_metric_extra(metric)
    make_ssim()
    from . import seg_oracle as seg
    a4 = torch.ones(4)
    make_net(nets, losses, seg, "vnet3d_bin_16", "vnet", 3, lambda: nets.VNet3d(1, 1), (2, 1, 16, 16, 16), 1,
             losses.BinaryDiceLoss())
    make_net(nets, losses, seg, "unet3d_mc4_16", "unet", 3, lambda: nets.UNet3d(1, 4), (1, 1, 16, 16, 16), 4,
             losses.MutilDiceLoss(a4))
    make_net(nets, losses, seg, "vnet2d_mc2_32", "vnet", 2, lambda: nets.VNet2d(1, 2), (2, 1, 32, 32), 2,
             losses.MutilCrossEntropyLoss(torch.ones(2)))
    make_net(nets, losses, seg, "unet2d_bin_32", "unet", 2, lambda: nets.UNet2d(1, 1), (2, 1, 32, 32), 1,
             losses.BinaryCrossEntropyDiceLoss())


if __name__ == "__main__":
    main()
