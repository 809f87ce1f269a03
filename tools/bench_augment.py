"""Times the batch launch of the on-device augmentation (seg_augment3d, csrc/augment.hip) on the VNet3d training batch of BASELINE: 4 x 1 x 96^3 float32
plus a uint8 label, (N, C, D, H, W), with the DataAug3D defaults (rotation 5 degrees, shifts 0.01, zoom 0.01, rescale 1.1, horizontal flip) and the
same with rotation 20 degrees (a wider gather footprint).

    python tools/bench_augment.py [--reps 50] [--host-reps 2] [--out FILE]

device: seg_augment3d through the C-ABI on resident tensors, outputs, workspace and parameters (nothing allocated in the timed window), --inner calls
        back to back between two hip events so that the queue stays fed, time per call = window / inner; warm-up first, median of --reps windows.
copy:   a device-to-device copy of the same number of bytes (image + label, read once and written once) in the same process, timed the same way: the
        floor of any kernel that moves these bytes.
host:   what the reference does per sample - scipy.ndimage.affine_transform(order=0) per channel for image and label, the flips, the rescale - restated
        here because the reference tree is not part of this repository; scipy runs it on ONE core; median of --host-reps over the same batch and draws.
One JSON line with both settings (profiles/augment3d_bench.json is such a line); nothing is timed on the host checker."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_reference(x, y, draws, rescale):
    """images_masks_3dtransform.py:43-53, 187-269 + standardize for a channel-first batch, with scipy; returns the transformed batch"""
    from scipy import ndimage
    xo, yo = np.empty_like(x), np.empty_like(y)
    for k, (m, flips, _) in enumerate(draws):
        vols = [ndimage.affine_transform(v, m[:, :3], m[:, 3], order=0, mode="nearest", cval=0.) for v in list(x[k]) + [y[k]]]
        for axis in range(3):
            if flips[axis]:
                vols = [np.flip(v, axis) for v in vols]
        xo[k] = np.stack(vols[:-1]) * np.float32(rescale)
        yo[k] = vols[-1]
    return xo, yo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D, draw_transform, pack_params, transform_batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")
    lib = _capi.lib_for(dev)
    n, s = a.batch, a.size
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, 1, s, s, s)).astype(np.float32)
    y = (rng.random((n, s, s, s)) < 0.3).astype(np.uint8) * 255
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    nbytes = x.nbytes + y.nbytes
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)

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

    copy_ms = timed(lambda: dst.copy_(src))
    lines = []
    for rotation in (5, 20):
        gen = ImageDataGenerator3D(rotation_range=rotation, width_shift_range=0.01, height_shift_range=0.01, depth_shift_range=0.01, zoom_range=0.01,
                                   rescale=1.1, horizontal_flip=True)
        np.random.seed(rotation)
        draws = [draw_transform(gen, (s, s, s, 1)) for _ in range(n)]
        params = pack_params(np.stack([d[0] for d in draws]), np.array([d[1] for d in draws]))
        pd = torch.from_numpy(params).to(dev)
        xo, yo = torch.empty_like(xd), torch.empty_like(yd)
        ws = torch.empty(int(lib.seg_augment3d_ws_bytes(n)) + 256, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
        st = _capi.stream_for(dev)

        def call():
            lib.check(lib.seg_augment3d(xd.data_ptr(), xo.data_ptr(), n, 1, s, s, s, s * s * s, 1, yd.data_ptr(), yo.data_ptr(), 0, 1, params.ctypes.data,
                                        pd.data_ptr(), 0, 0.0, 0.0, 1.1, 0, wsp, st), "seg_augment3d")
        ms = timed(call)
        out = dict(zip("xy", transform_batch(xd, params, yd, "th", "nearest", 0., None, 1.1, False, params_dev=pd)))      # the package's own path
        assert torch.equal(out["x"], xo) and torch.equal(out["y"], yo)
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            want = host_reference(x, y, draws, 1.1)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(out["x"].cpu().numpy(), want[0]) and np.array_equal(out["y"].cpu().numpy(), want[1])
        dev_ms, cp_ms, h_ms = statistics.median(ms), statistics.median(copy_ms), statistics.median(host_ms)
        line = {"batch": [n, 1, s, s, s], "label": "uint8", "rotation_deg": rotation, "bytes_read_plus_written": 2 * nbytes,
                "device_call_ms_median": round(dev_ms, 4), "device_call_ms_min": round(min(ms), 4), "device_call_ms_max": round(max(ms), 4),
                "device_GBps": round(2 * nbytes / (dev_ms * 1e-3) / 1e9, 1), "reps": a.reps, "calls_per_window": a.inner,
                "d2d_copy_same_bytes_ms_median": round(cp_ms, 4), "call_over_copy": round(dev_ms / cp_ms, 2),
                "host_scipy_ms_median": round(h_ms, 1), "host_cores_used": 1, "host_reps": a.host_reps, "host_over_call": round(h_ms / dev_ms, 1),
                "volumes_per_s_device": round(n / (dev_ms * 1e-3), 1), "volumes_per_s_host": round(n / (h_ms * 1e-3), 2),
                "equal_to_host": True, "build": lib.build_info()}
        lines.append(line)
    text = json.dumps({"bench": "augment3d", "runs": lines})
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
