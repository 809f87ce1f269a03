"""Times the batch launch of the on-device 2-D augmentation (seg_augment2d, csrc/augment2d.hip) on the VNet2d training batch of BASELINE config C2:
16 x 1 x 512^2 float32 plus a uint8 label, (N, C, H, W), mirror border.

    python tools/bench_augment2d.py [--reps 50] [--out profiles/augment2d_bench.json]

Variants, all timed in the same call and the same way - seg_augment2d through the C-ABI on resident tensors, outputs and parameters (nothing allocated
in the timed window), --inner calls back to back between two hip events so that the queue stays fed, time per call = window / inner; warm-up first,
median of --reps windows:
  identity   every sample: no flip, no blur, no warp, no tone (the 16-byte copy path)
  default    one seeded draw per sample with the default probabilities of Segmenation_Aug
  motion7    every sample: a 7 x 7 motion blur (7 taps) evaluated at the four taps of a warp
  copy       a torch device-to-device copy of the same number of bytes (image + label, read once and written once): the floor of any kernel that
             moves these bytes
No time is fixed in advance; the ratios to the copy are what DESIGN.md quotes.  One JSON line; nothing is timed on the host checker."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd import augment2d as a2
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment2d: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")
    lib = _capi.lib_for(dev)
    n, s = a.batch, a.size
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, 1, s, s)).astype(np.float32)
    y = (rng.random((n, s, s)) < 0.3).astype(np.uint8) * 255
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    xo, yo = torch.empty_like(xd), torch.empty_like(yd)
    nbytes = x.nbytes + y.nbytes
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = _capi.stream_for(dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        return ms

    np.random.seed(0)
    variants = {
        "identity": [a2.make_params2d() for _ in range(n)],
        "default": [a2.draw_transform2d(a2.Segmenation_Aug(), (s, s)) for _ in range(n)],
        "motion7": [a2.make_params2d(a2.affine_matrix2d(-40 + 5.0 * k, 0.8 + 0.025 * k, 3.0 * k - 20, 11 - 2.0 * k, (s, s)), hflip=bool(k & 1),
                                     blur=1, kernel=a2.motion_kernel(7, (0, k % 7), (6, 6 - k % 7))) for k in range(n)],
    }
    copy_ms = statistics.median(timed(lambda: dst.copy_(src)))
    runs = []
    for name, blocks in variants.items():
        params = a2.pack_params2d(blocks)
        pd = torch.from_numpy(params).to(dev)

        def call():
            lib.check(lib.seg_augment2d(xd.data_ptr(), xo.data_ptr(), n, 1, s, s, s * s, s * s, 1, yd.data_ptr(), yo.data_ptr(), 0, params.ctypes.data,
                                        pd.data_ptr(), a2.BORDER_MODES["mirror"], 0.0, 0.0, None, st), "seg_augment2d")
        ms = timed(call)
        out = a2.transform_batch2d(xd, params, yd, "th", "mirror", params_dev=pd)      # the package's own path gives the same bytes
        assert torch.equal(out[0], xo) and torch.equal(out[1], yo)
        if name == "identity":
            assert torch.equal(xo, xd) and torch.equal(yo, yd)
        med = statistics.median(ms)
        runs.append({"variant": name, "steps": {"flip": int(sum(p[6] != 0 for p in blocks)), "blur": int(sum(p[8] != 0 for p in blocks)),
                                                "warp": int(sum(p[7] != 0 for p in blocks)), "tone": int(sum(p[10] != 1 or p[11] != 0 for p in blocks))},
                     "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4),
                     "GBps": round(2 * nbytes / (med * 1e-3) / 1e9, 1), "call_over_copy": round(med / copy_ms, 2)})
    text = json.dumps({"bench": "augment2d", "batch": [n, 1, s, s], "label": "uint8", "border": "mirror", "bytes_read_plus_written": 2 * nbytes,
                       "reps": a.reps, "calls_per_window": a.inner, "d2d_copy_same_bytes_ms_median": round(copy_ms, 4), "runs": runs,
                       "build": lib.build_info()})
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
