"""Writes tests/golden/surface_metric.npz: what the LIVE reference class Seg_Metirc3d (model/metric.py:11-142, loaded as is through
oracle.ref_loader) computes for the cases of tests/test_surface_metric.py.  Numeric data only: bit-packed masks, shapes, spacings, the nine metric
values, the surface voxel indices in the reference's order (numpy.nonzero: raster order) and both nearest-distance arrays.

    python tools/make_surface_golden.py            (needs the reference tree and scipy)

tests/test_surface_metric.py::test_golden_file_is_what_the_live_reference_computes re-runs `reference_results` and compares with the file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "surface_metric.npz")
SPACINGS = ((1.0, 1.0, 1.0), (0.78, 0.78, 2.5))          # (x, y, z), as the reference's constructor takes it
METRICS = ("dice", "jaccard", "VOE", "RVD", "FNR", "FPR", "ASSD", "RMSD", "MSD")


def ellipsoid(shape, centre, radii):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1.0


def make_cases():
    """[(name, real, pred)] bool masks from a seeded generator: an off-centre ellipsoid on each side + salt noise on the prediction"""
    rng = np.random.default_rng(20240611)
    salt = lambda shape, p: rng.random(shape) < p
    cases = []
    # every extent below one wave, both masks touch volume faces, surfaces smaller than one LDS tile
    s = (5, 7, 9)
    cases.append(("tiny_5x7x9", ellipsoid(s, (1.5, 3.0, 3.5), (3.0, 4.5, 5.0)), ellipsoid(s, (2.5, 4.0, 5.5), (3.0, 3.5, 4.5)) | salt(s, 0.01)))
    # W no multiple of 64, D = 3: every mask voxel has an out-of-volume neighbour along z; many tiles, target list split over workgroups
    s = (3, 130, 67)
    cases.append(("slab_3x130x67", ellipsoid(s, (1.0, 62.0, 31.0), (4.0, 72.0, 37.0)), ellipsoid(s, (1.0, 80.0, 40.0), (4.0, 36.0, 21.0)) | salt(s, 0.01)))
    # an interior blob against salt noise
    s = (12, 20, 70)
    cases.append(("blob_12x20x70", ellipsoid(s, (5.5, 9.5, 33.0), (5.0, 9.0, 31.0)), ellipsoid(s, (6.0, 11.0, 40.0), (3.0, 5.0, 12.0)) | salt(s, 0.14)))
    # one voxel against the full volume: one query point against a 96-point shell
    s = (4, 5, 6)
    one = np.zeros(s, dtype=bool)
    one[1, 2, 2] = True
    cases.append(("voxel_4x5x6", one, np.ones(s, dtype=bool)))
    return cases


def reference_results(ref_metric, real, pred, spacing):
    """the reference class on one pair of bool masks -> dict of arrays"""
    m = ref_metric.Seg_Metirc3d(real, pred, spacing)
    values = [m.get_dice_coefficient()[0], m.get_jaccard_index(), m.get_VOE(), m.get_RVD(), m.get_FNR(), m.get_FPR(), m.get_ASSD(), m.get_RMSD(), m.get_MSD()]
    d, h, w = real.shape
    zyx = np.array(spacing[::-1]).reshape(1, 3)

    def index(pts):
        v = np.rint(pts / zyx).astype(np.int64)
        return ((v[:, 0] * h + v[:, 1]) * w + v[:, 2]).astype(np.int32)

    return {"values": np.array(values, dtype=np.float64), "surf_real": index(m.real_mask_surface_pts), "surf_pred": index(m.pred_mask_surface_pts),
            "nn_r2p": np.asarray(m.real2pred_nn, dtype=np.float64), "nn_p2r": np.asarray(m.pred2real_nn, dtype=np.float64)}


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader
    ref_metric = ref_loader.load()[2]
    out = {"spacings": np.array(SPACINGS), "names": np.array([c[0] for c in make_cases()])}
    for i, (name, real, pred) in enumerate(make_cases()):
        out["c%d_shape" % i] = np.array(real.shape, dtype=np.int32)
        out["c%d_real" % i] = np.packbits(real.ravel())
        out["c%d_pred" % i] = np.packbits(pred.ravel())
        for j, sp in enumerate(SPACINGS):
            r = reference_results(ref_metric, real, pred, sp)
            for k, v in r.items():
                if k.startswith("surf_"):
                    if j == 0:
                        out["c%d_%s" % (i, k)] = v
                    else:
                        assert np.array_equal(out["c%d_%s" % (i, k)], v)
                else:
                    out["c%d_s%d_%s" % (i, j, k)] = v
            print("%-14s spacing %-16s surface %5d / %5d  %s" % (name, sp, len(r["surf_real"]), len(r["surf_pred"]),
                                                                 " ".join("%s %.6g" % kv for kv in zip(METRICS, r["values"]))))
    v = out["c3_s0_values"]
    assert abs(v[6] - 2.676301764188125) < 1e-15 and abs(v[8] - 4.123105625617661) < 1e-15, (v[6], v[8])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
