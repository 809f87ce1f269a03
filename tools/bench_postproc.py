"""Times the on-device mask cleaning (csrc/postproc.hip) on synthetic organ masks: a few blobs plus 1 % salt noise, fixed seed, uint8, at
256 x 256 x 256 and 512 x 512 x 300.

    python tools/bench_postproc.py [--reps 30] [--host-reps 1] [--out FILE]

device: keep_largest_component (faces) = seg_cc_filter, and binary_morphology(open, ball 2) = seg_morph3d, through the C-ABI on resident tensors and
        workspace (nothing allocated in the timed window), --inner calls back to back between two hip events, time per call = window / inner;
        warm-up first, median / min / max of --reps windows.
copy:   a device-to-device copy of the same bytes (the mask read once, written once) in the same process, timed the same way: the floor of any
        kernel that moves these bytes.
host:   scipy.ndimage on ONE core for the same operation on the smaller volume (label + bincount + compare; binary_opening with the same ball);
        the device results are compared with it.
One JSON line (profiles/postproc_bench.json is such a line); nothing is timed on the host checker."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def organ_mask(shape, seed=0):
    """a few ellipsoid blobs plus 1 % salt noise"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.ogrid[:d, :h, :w]
    m = np.zeros(shape, bool)
    for _ in range(5):
        c = rng.random(3) * 0.6 + 0.2
        r = rng.random(3) * 0.15 + 0.08
        m |= ((z / d - c[0]) / r[0]) ** 2 + ((y / h - c[1]) / r[1]) ** 2 + ((x / w - c[2]) / r[2]) ** 2 <= 1.0
    m |= rng.random(shape) < 0.01
    return m.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pytorchdeeplearing_amd import _capi
    from make_postproc_golden import morph_ref, structure
    if not torch.cuda.is_available():
        raise SystemExit("bench_postproc: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")
    lib = _capi.lib_for(dev)
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

    def summary(ms):
        return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    runs = []
    for k, shape in enumerate(((256, 256, 256), (512, 512, 300))):
        mask = organ_mask(shape)
        md = torch.from_numpy(mask).to(dev)
        out = torch.empty_like(md)
        nd = (1,) + shape
        ws = torch.empty(int(max(lib.seg_cc_ws_bytes(*nd), lib.seg_morph3d_ws_bytes(*nd))) + 256, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() + (-ws.data_ptr()) % 256
        src, dst = torch.empty_like(md), torch.empty_like(md)
        copy_ms = timed(lambda: dst.copy_(src))

        def largest():
            lib.check(lib.seg_cc_filter(md.data_ptr(), out.data_ptr(), *nd, -1, 1, 0, 0, wsp, None, st), "seg_cc_filter")

        def opening():
            lib.check(lib.seg_morph3d(md.data_ptr(), out.data_ptr(), *nd, -1, 2, 0, 2, 2, 2, -1, 1, wsp, st), "seg_morph3d")
        line = {"shape": list(shape), "voxels": int(mask.size), "foreground": int(mask.sum()), "d2d_copy_same_bytes": summary(copy_ms)}
        cp = statistics.median(copy_ms)
        for name, fn in (("keep_largest_faces", largest), ("open_ball2", opening)):
            ms = timed(fn)
            line[name] = dict(summary(ms), over_copy=round(statistics.median(ms) / cp, 2),
                              GBps_mask_read_plus_written=round(2 * mask.size / (statistics.median(ms) * 1e-3) / 1e9, 1))
            fn()
            line[name + "_result"] = out.cpu().numpy().copy()
        if k == 0:                                              # the host leg: the smaller volume only
            from scipy import ndimage
            host = {}
            for name in ("keep_largest_faces", "open_ball2"):
                t = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    if name == "keep_largest_faces":
                        lab, _ = ndimage.label(mask)
                        want = (lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))).astype(np.uint8)
                    else:
                        want = morph_ref(mask.astype(bool), "open", structure("ball", (2, 2, 2))[0]).astype(np.uint8)
                    t.append((time.perf_counter() - t0) * 1e3)
                host[name] = want
                line[name]["host_scipy_ms_median"] = round(statistics.median(t), 1)
                line[name]["host_over_device"] = round(statistics.median(t) / line[name]["ms_median"], 1)
                line[name]["equal_to_host"] = bool(np.array_equal(line[name + "_result"], want))
            line["host_cores_used"] = 1
        for name in ("keep_largest_faces", "open_ball2"):
            del line[name + "_result"]
        runs.append(line)
    text = json.dumps({"bench": "postproc", "reps": a.reps, "calls_per_window": a.inner, "build": lib.build_info(), "runs": runs})
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
