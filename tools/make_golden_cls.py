"""Writes the classifier goldens from the LIVE reference (loaded as is through oracle.ref_loader; CPU):

    tests/golden/resnet_modules.json      state_dict keys / shapes / leaf-module order of ResNet3d / ResNet2d, SHA-256 of every tensor after
                                          `manual_seed(s); apply(initialize_weights)`, calc_accuracy values, what datasetModelClassifywithnpy returns
    tests/golden/<case>.npz               per case of tests/cls_oracle.CASES: eval logits / loss / 18-column gradient summaries, and a train-mode step
                                          with the dropout masks the reference drew (the layout of vnet3d_bin_16.npz)

    python tools/make_golden_cls.py       (needs the reference tree)

Numeric data and names only.  Parameters are NOT stored: both sides derive them from a seed (cls_oracle.seeded_params).  Two shims, of the kind
ref_loader applies for VNet3d.feature (no reference file is edited):
  * the reference's DownTransition3d / 2d read a module global `prob` that is never defined, so ResNet3d(1, 1) raises NameError as shipped; `prob = 0.2`
    (the VNet value) is set on the two modules before construction;
  * in train mode the reference's backward pass raises ("modified by an inplace operation"): DownTransition applies the in-place dropout `do1` to the output
    of its in-place ReLU, which autograd saved for the ReLU's backward.  For the train-mode step only, `relu1` of the four DownTransitions is replaced by
    `x.clamp(min=0)` - the same values, and a backward that reads its input instead of its output, so the in-place dropout behind it is legal.  The forward
    pass (and with it the train logits and the masks) is what the unmodified reference computes."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                   # noqa: E402
from oracle.make_golden import grad_summary, tensor_sha256      # noqa: E402
import cls_oracle                                               # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SKIPPED_LEAVES = ("ReLU", "Dropout3d", "Dropout2d", "GlobalAveragePooling")       # parameter-free leaves the engine folds away
MODULES = (("ResNet3d", (1, 2)), ("ResNet2d", (3, 1)))
INITS = (("ResNet3d", (1, 2), 110), ("ResNet2d", (1, 3), 111))
PROB = 0.2


class _ClampRelu(torch.nn.Module):
    def forward(self, x):
        return x.clamp(min=0)


def load_reference():
    nets, losses, metric = ref_loader.load()
    for name in ("ResNet3d", "ResNet2d"):
        sys.modules["ref_networks." + name].prob = PROB
    return nets, losses, metric


def accuracy_cases():
    """(name, input, target): what the wrappers hand to calc_accuracy - arg-max indices against (N,) labels, and the binary form, an (N, 1) tensor of
    thresholded probabilities against (N,) labels, which broadcasts to (N, N)"""
    g = torch.Generator().manual_seed(5)
    cases = []
    for n, c in ((4, 3), (7, 5)):
        cases.append(("multi_%d_%d" % (n, c), torch.randint(0, c, (n,), generator=g), torch.randint(0, c, (n,), generator=g)))
    for n in (1, 4, 6):
        cases.append(("binary_%d" % n, (torch.rand((n, 1), generator=g) > 0.5).float(), (torch.rand((n,), generator=g) > 0.5).float()))
    return cases


def make_modules(nets, metric):
    out = {"prob": PROB, "tree": [], "init": [], "accuracy": [], "dataset_npy": None}
    for cls, args in MODULES:
        m = getattr(nets, cls)(*args)
        sd = m.state_dict()
        out["tree"].append({"cls": cls, "args": list(args), "keys": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()],
                            "numel": int(sum(v.numel() for v in sd.values())),
                            "leaves": [type(x).__name__ for x in m.modules() if not list(x.children()) and type(x).__name__ not in SKIPPED_LEAVES]})
    for cls, args, seed in INITS:
        m = getattr(nets, cls)(*args)
        torch.manual_seed(seed)
        m.apply(nets.initialize_weights)
        out["init"].append({"cls": cls, "args": list(args), "seed": seed, "sha256": {k: tensor_sha256(v) for k, v in m.state_dict().items()}})
    for name, a, b in accuracy_cases():
        out["accuracy"].append({"name": name, "input": a.tolist(), "target": b.tolist(), "value": float(metric.calc_accuracy(a, b))})
    # the .npy dataset (model/dataset.py:8-39) on a generated volume; the module imports cv2 at its top, which the .npy class never calls
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_model.dataset", os.path.join(ref_loader.REF, "model", "dataset.py"))
    ds = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ds)
    with tempfile.TemporaryDirectory() as d:
        vol = np.random.default_rng(3).normal(size=(4, 6, 8)).astype(np.float64)
        path = os.path.join(d, "v.npy")
        np.save(path, vol)
        item = ds.datasetModelClassifywithnpy([path], ["1"], targetsize=(1, 4, 6, 8))[0]
        out["dataset_npy"] = {"volume_shape": [4, 6, 8], "seed": 3, "image_dtype": str(item["image"].dtype), "image_shape": list(item["image"].shape),
                              "label_dtype": str(item["label"].dtype), "label_shape": list(item["label"].shape), "label": int(item["label"]),
                              "image_sha256": tensor_sha256(item["image"])}
    with open(os.path.join(OUT, "resnet_modules.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("modules:", [(t["cls"], len(t["keys"]), t["numel"]) for t in out["tree"]])


def make_case(nets, losses, tag, ndim, shape, numclass, loss_name, seed):
    m = getattr(nets, "ResNet%dd" % ndim)(shape[1], numclass)
    params = cls_oracle.seeded_params(m, nets.initialize_weights, seed)
    res = m.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x, y = cls_oracle.batch(shape, numclass)
    alpha = [1.] * numclass
    loss_mod = {"BinaryCrossEntropyLoss": lambda: losses.BinaryCrossEntropyLoss(), "BinaryFocalLoss": lambda: losses.BinaryFocalLoss(alpha=0.25, gamma=2),
                "MutilCrossEntropyLoss": lambda: losses.MutilCrossEntropyLoss(alpha=alpha), "MutilFocalLoss": lambda: losses.MutilFocalLoss(alpha=alpha)}[loss_name]()
    out = dict(x_sum=np.float64(x.double().sum()), y=y.numpy(), seed=np.int64(seed))
    names = [k for k, _ in m.named_parameters()]
    out["grad_names"] = np.array(names)
    m.eval()
    logits = m(x)
    loss = loss_mod(logits, y)
    m.zero_grad()
    loss.backward()
    out["eval_logits"], out["eval_loss"] = logits.detach().numpy(), loss.detach().numpy()
    out["grad_summary"] = np.stack([grad_summary(p.grad) for _, p in m.named_parameters()])
    masks = []

    def pre(mod, inp):           # peek the CPU generator in front of every dropout call: the module then consumes the same draws
        n, c = inp[0].shape[:2]
        state = torch.get_rng_state()
        mk = torch.empty((n, c) + (1,) * (inp[0].dim() - 2)).bernoulli_(1 - PROB).div_(1 - PROB)
        torch.set_rng_state(state)
        masks.append(mk.reshape(n, c).clone())

    for mod in m.modules():
        if type(mod).__name__.startswith("DownTransition"):
            mod.relu1 = _ClampRelu()
    hooks = [mod.register_forward_pre_hook(pre) for mod in m.modules() if isinstance(mod, (torch.nn.Dropout3d, torch.nn.Dropout2d))]
    m.train()
    torch.manual_seed(99)
    logits_t = m(x)
    loss_t = loss_mod(logits_t, y)
    m.zero_grad()
    loss_t.backward()
    for h in hooks:
        h.remove()
    out["train_logits"], out["train_loss"] = logits_t.detach().numpy(), loss_t.detach().numpy()
    out["train_grad_summary"] = np.stack([grad_summary(p.grad) for _, p in m.named_parameters()])
    out["train_masks"] = np.stack([np.pad(k.numpy(), ((0, 0), (0, 256 - k.shape[1]))) for k in masks]).astype(np.float16)
    out["train_mask_channels"] = np.array([k.shape[1] for k in masks])
    np.savez_compressed(os.path.join(OUT, tag + ".npz"), **out)
    print(tag, "logits", logits.detach().reshape(-1).tolist(), "loss", float(loss), "train loss", float(loss_t), "masks", [k.shape[1] for k in masks],
          "dropped", [int((k == 0).sum()) for k in masks])


def main():
    if not ref_loader.available():
        sys.exit("reference tree not available; the goldens can only be regenerated where it is")
    torch.set_num_threads(1)
    nets, losses, metric = load_reference()
    make_modules(nets, metric)
    for case in cls_oracle.CASES:
        make_case(nets, losses, *case)


if __name__ == "__main__":
    main()
