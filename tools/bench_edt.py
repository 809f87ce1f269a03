"""Times seg_edt (the exact Euclidean distance transform on the device, csrc/edt.hip) against a device copy of the same bytes and against
scipy.ndimage.distance_transform_edt on the host, on the ellipsoid pair of tools/bench_surface_metric.py at 96^3 and 160^3 and on a batch of 16 ellipses of
512^2 run as d = 1.

    python tools/bench_edt.py [--sizes 96 160] [--no-2d] [--reps 30] [--host-reps 3] [--out FILE]

device: one C call (every launch of it) per repetition on resident uint8 volumes, hip events around each call, warm-up first, median of --reps; modes
        SEG_EDT_DISTANCE (one transform) and SEG_EDT_BOUNDARY (the mask and its complement), with the anisotropic spacing (the f32 path) and mode 1 with
        unit spacing as well (the integer path), on the clean mask (`real`) and on the one with 1 % salt noise (`pred`).
copy:   out.copy_(src) of the same 4 bytes per voxel, timed the same way - the rate the row pass could reach, and the yardstick for the column passes.
host:   scipy on the same mask and spacing, median of --host-reps (per sample, as a data-loader worker would run it).
One JSON line per size."""
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

from bench_surface_metric import ellipsoid, make_pair          # noqa: E402

SPACING = (2.5, 0.78, 0.78)          # (sz, sy, sx)


def ellipse_batch(n=16, size=512, seed=0):
    """n ellipses of size^2, each a little different, as (real, pred) like make_pair: pred carries 1 % salt noise"""
    rng = np.random.default_rng(seed)
    real = np.stack([ellipsoid((1, size, size), (0.0, (0.45 + 0.01 * i) * size, 0.52 * size), (1.0, (0.25 + 0.005 * i) * size, 0.33 * size)) for i in range(n)])
    return real, real | (rng.random(real.shape) < 0.01)


def timed(call, reps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[96, 160])
    ap.add_argument("--no-2d", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    from pytorchdeeplearing_amd import _capi, prepost
    if not torch.cuda.is_available():
        raise SystemExit("bench_edt: needs the GPU (nothing is timed on the host checker)")
    dev = torch.device("cuda:0")
    lib = _capi.lib_for(dev)
    jobs = [("%d^3" % n, tuple(m[None] for m in make_pair(n))) for n in a.sizes]
    if not a.no_2d:
        jobs.append(("16x512^2", ellipse_batch()))
    lines = []
    for tag, pair in jobs:
        nd = tuple(pair[0].shape)
        voxels = int(np.prod(nd))
        nbytes = lib.seg_edt_ws_bytes(*nd)
        lib.check(nbytes, "seg_edt_ws_bytes")
        ws = prepost._pp_workspace(dev, nbytes)
        out = torch.empty(nd, dtype=torch.float32, device=dev)
        src = torch.rand(nd, dtype=torch.float32, device=dev)
        copy_ms, _ = timed(lambda: out.copy_(src), a.reps, a.warmup)
        line = {"size": tag, "shape_ndhw": list(nd), "voxels": voxels, "spacing_zyx": list(SPACING), "reps": a.reps, "copy_4B_per_voxel_ms_median": copy_ms,
                "copy_GBps": round(8.0 * voxels / (copy_ms * 1e-3) / 1e9, 1)}
        for name, mask in zip(("real", "pred"), pair):
            t = torch.from_numpy(mask.astype(np.uint8)).to(dev)

            def call(mode, sp):
                lib.check(lib.seg_edt(t.data_ptr(), *nd, -1, *sp, mode, ws.data_ptr(), out.data_ptr(), voxels // nd[0], _capi.stream_for(dev)), "seg_edt")

            rec = {"foreground_fraction": round(float(mask.mean()), 4)}
            for key, mode, sp in (("distance_unit", prepost.EDT_DISTANCE, (1.0, 1.0, 1.0)), ("distance_aniso", prepost.EDT_DISTANCE, SPACING),
                                  ("boundary_aniso", prepost.EDT_BOUNDARY, SPACING)):
                med, lo = timed(lambda: call(mode, sp), a.reps, a.warmup)
                rec[key + "_ms_median"], rec[key + "_ms_min"] = med, lo
                rec[key + "_Mvoxel_per_s"] = round(voxels / (med * 1e-3) / 1e6, 1)
            call(prepost.EDT_DISTANCE, SPACING)
            got = out.cpu().numpy()
            host_ms = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                want = np.stack([ndimage.distance_transform_edt(s, sampling=SPACING) for s in mask])
                host_ms.append((time.perf_counter() - t0) * 1e3)
            nz = want > 0
            rel = float(np.max(np.abs(got[nz] - want[nz]) / want[nz]))
            assert rel < 1e-5 and not got[~nz].any(), (tag, name, rel)
            rec["host_scipy_ms_median"] = round(statistics.median(host_ms), 2)
            rec["speedup_distance_aniso_vs_host"] = round(rec["host_scipy_ms_median"] / rec["distance_aniso_ms_median"], 1)
            rec["distance_aniso_over_copy"] = round(rec["distance_aniso_ms_median"] / copy_ms, 1)
            rec["max_rel_dev_vs_scipy"] = rel
            line[name] = rec
        line["host_reps"] = a.host_reps
        line["build"] = lib.build_info()
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
