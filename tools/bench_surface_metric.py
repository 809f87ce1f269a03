"""Times seg_surface_metrics (Seg_Metirc3d on the device, csrc/surface.hip) against the host path of the reference, on the two VNet3d volume sizes of
BASELINE: an off-centre ellipsoid pair with 1 % salt noise on the prediction at 96^3 and 160^3.

    python tools/bench_surface_metric.py [--sizes 96 160] [--reps 30] [--host-reps 3] [--out FILE]

device: one C call (all six launches) per repetition on resident uint8 volumes, hip events around each call, warm-up first, median of --reps.
host:   the reference's algorithm with scipy (binary_erosion with the 18-neighbourhood ^ mask, two cKDTree builds + queries, the three distance
        numbers), written out here because the reference tree is not part of this repository; median of --host-reps, on the same masks.
The pair count of the all-pairs pass is 2 * n_surf_real * n_surf_pred; the pair rate printed is pairs over the WHOLE call (surface extraction and the
reductions included), i.e. a lower bound of the search kernel's own rate - `rocprofv3 --kernel-trace --stats` of this script gives
surf_nn_kernel alone.  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ellipsoid(shape, centre, radii):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1.0


def make_pair(n, seed=0):
    rng = np.random.default_rng(seed)
    s = (n, n, n)
    real = ellipsoid(s, (0.47 * n, 0.5 * n, 0.52 * n), (0.30 * n, 0.36 * n, 0.33 * n))
    pred = ellipsoid(s, (0.50 * n, 0.46 * n, 0.55 * n), (0.28 * n, 0.35 * n, 0.36 * n)) | (rng.random(s) < 0.01)
    return real, pred


def host_reference(real, pred, spacing):
    """model/metric.py:34-65, 121-142 restated with scipy: (ASSD, RMSD, MSD, n_surf_real, n_surf_pred)"""
    from scipy import ndimage, spatial
    kernel = ndimage.generate_binary_structure(3, 2)
    zyx = np.array(spacing[::-1]).reshape(1, 3)
    pts = [np.argwhere(ndimage.binary_erosion(m, kernel) ^ m) * zyx for m in (real, pred)]
    r2p = spatial.cKDTree(pts[1]).query(pts[0])[0]
    p2r = spatial.cKDTree(pts[0]).query(pts[1])[0]
    n = len(pts[0]) + len(pts[1])
    return (r2p.sum() + p2r.sum()) / n, float(np.sqrt(((r2p ** 2).sum() + (p2r ** 2).sum()) / n)), max(r2p.max(), p2r.max()), len(pts[0]), len(pts[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 160])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pytorchdeeplearing_amd import _capi, metric
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_metric: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")
    lib = _capi.lib_for(dev)
    spacing = (0.78, 0.78, 2.5)
    lines = []
    for n in a.sizes:
        real, pred = make_pair(n)
        r = torch.from_numpy(real.astype(np.uint8)).to(dev)
        p = torch.from_numpy(pred.astype(np.uint8)).to(dev)
        ws = metric._surface_ws(lib, (n, n, n), dev)
        out = torch.empty(16, dtype=torch.float64, device=dev)
        nn = [torch.empty(r.numel(), dtype=torch.float32, device=dev) for _ in range(2)]
        call = lambda: metric._surface_call(lib, r, p, -1, spacing[::-1], ws, out, nn[0], nn[1])
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        o = out.cpu().numpy()
        t0 = time.perf_counter()
        m = metric.Seg_Metirc3d(r, p, spacing)
        got = (m.get_ASSD(), m.get_RMSD(), m.get_MSD())
        class_ms = (time.perf_counter() - t0) * 1e3           # constructor (allocations, call, read-back) + the three getters, from resident tensors
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            want = host_reference(real, pred, spacing)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        rel = max(abs(g - w) / w for g, w in zip(got, want[:3]))
        assert (int(o[4]), int(o[5])) == want[3:] and rel < 1e-5, (o[:6], got, want)
        pairs = 2.0 * o[4] * o[5]
        dev_ms = statistics.median(ms)
        line = {"size": n, "n_surf_real": int(o[4]), "n_surf_pred": int(o[5]), "pairs": pairs, "device_call_ms_median": round(dev_ms, 4),
                "device_call_ms_min": round(min(ms), 4), "device_call_ms_max": round(max(ms), 4), "reps": a.reps,
                "pairs_per_s_whole_call": pairs / (dev_ms * 1e-3), "class_from_resident_tensors_ms": round(class_ms, 3),
                "host_scipy_ms_median": round(statistics.median(host_ms), 2), "host_reps": a.host_reps,
                "speedup_call_vs_host": round(statistics.median(host_ms) / dev_ms, 1), "max_rel_dev_ASSD_RMSD_MSD_vs_host": rel,
                "build": lib.build_info()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
