"""Times one optimisation step of the classifiers (seg_train_step on SEG_NET_RESNET) at ResNet3d 4 x 1 x 96^3 and ResNet2d 16 x 1 x 512^2 in f16:
HIP events around every step, warm-up first, median of --reps (>= 50) steps.

    python tools/bench_resnet.py [--reps 50] [--warmup 10] [--out FILE]

Beside each figure, in the same process and for orientation only:
  vnet:   the same-shape VNet step on this binary (the encoder is the VNet's; the classifier drops the decoder);
  torch:  stock PyTorch autocast (f16, GradScaler, torch.optim.Adam) on an in-file torch module of the same structure - the structure restated here,
          because no reference tree exists where this runs;
  head:   the share of the step inside the classification-head kernels (profiling class cls_head; a separate profiled step).
One JSON line (profiles/resnet_bench.json is such a line); nothing is timed on the host checker."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_resnet(ndim, in_ch, numclass):
    import torch
    from torch import nn
    Conv = nn.Conv3d if ndim == 3 else nn.Conv2d
    Drop = nn.Dropout3d if ndim == 3 else nn.Dropout2d

    class Unit(nn.Module):
        def __init__(self, cin, cout, k, stride=1):
            super().__init__()
            self.conv, self.gn = Conv(cin, cout, k, stride=stride, padding=1 if k == 3 else 0), nn.GroupNorm(8, cout)

        def forward(self, x):
            return torch.relu(self.gn(self.conv(x)))

    class Down(nn.Module):
        def __init__(self, cin, cout, n):
            super().__init__()
            self.down, self.ops, self.drop = Unit(cin, cout, 2, 2), nn.Sequential(*[Unit(cout, cout, 3) for _ in range(n)]), Drop(0.2)

        def forward(self, x):
            d = self.drop(self.down(x))
            return self.ops(d) + d

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c3, self.c1, self.gn = Conv(in_ch, 16, 3, padding=1), Conv(in_ch, 16, 1), nn.GroupNorm(8, 16)
            self.downs = nn.Sequential(Down(16, 32, 2), Down(32, 64, 3), Down(64, 128, 3), Down(128, 256, 3))
            self.fc = nn.Sequential(nn.Linear(256, 128), nn.ReLU(), nn.Linear(128, numclass))

        def forward(self, x):
            x = torch.relu(self.gn(self.c3(x))) + torch.relu(self.gn(self.c1(x)))
            x = self.downs(x)
            return self.fc(x.flatten(2).mean(2))
    return Net()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pytorchdeeplearing_amd import _capi, networks
    from pytorchdeeplearing_amd.engine import SegEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(a.reps, 50)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return round(statistics.median(ms), 4)

    res = {"build": _capi.lib_for(dev).build_info(), "dtype": "f16", "reps": max(a.reps, 50), "cases": []}
    for ndim, shape in ((3, (4, 1, 96, 96, 96)), (2, (16, 1, 512, 512))):
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g).to(dev)
        y = torch.randint(0, 2, (shape[0],), generator=g).to(dev)
        yseg = (torch.rand((shape[0],) + shape[2:], generator=g) > 0.8).to(torch.uint8).to(dev)
        case = {"net": "ResNet%dd" % ndim, "shape": list(shape)}
        torch.manual_seed(1)
        mod = getattr(networks, "ResNet%dd" % ndim)(1, 1, dtype="f16")
        mod.apply(networks.initialize_weights)
        e = SegEngine("resnet", ndim, 1, 1, dtype="f16", device=dev)
        e.load_state_dict(mod.state_dict())
        case["ms_per_step"] = timed(lambda: e.train_step(x, y, "BinaryCrossEntropyLoss", lr=1e-4, weight_decay=0.0, decoupled=False))
        e.profile_enable(["cls_head"])
        e.train_step(x, y, "BinaryCrossEntropyLoss", lr=1e-4, weight_decay=0.0, decoupled=False)
        torch.cuda.synchronize()
        p = e.profile_read().get("cls_head", {})
        e.profile_enable([])
        case["cls_head_launch_groups"], case["cls_head_ms"] = p.get("calls", 0), round(p.get("ms", 0.0), 4)
        del e
        v = SegEngine("vnet", ndim, 1, 1, dtype="f16", device=dev)
        vm = getattr(networks, "VNet%dd" % ndim)(1, 1, dtype="f16")
        torch.manual_seed(1)
        vm.apply(networks.initialize_weights)
        v.load_state_dict(vm.state_dict())
        case["vnet_ms_per_step"] = timed(lambda: v.train_step(x, yseg, "BinaryDiceLoss", lr=1e-4))
        del v
        net = torch_resnet(ndim, 1, 1).to(dev)
        net = net.to(memory_format=torch.channels_last_3d if ndim == 3 else torch.channels_last)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda")
        yf = y.float().reshape(-1, 1)

        def torch_step():
            with torch.autocast("cuda", dtype=torch.float16):
                loss = torch.nn.functional.binary_cross_entropy_with_logits(net(x).float(), yf)
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        case["torch_autocast_ms_per_step"] = timed(torch_step)
        del net, opt
        torch.cuda.empty_cache()
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
