"""Writes tests/golden/gradcam_2d.npz from the LIVE reference's GradCAM class (model/visualization.py:112-238, loaded as is; CPU):

    python tools/make_golden_gradcam.py       (needs the reference tree)

Cases: the two 2-D cases of tests/cls_oracle.CASES; layer sets down_tr256, down_tr64, in_tr and all five blocks; the first and the last class.  Per map
`<case>__<layer set>__c<class>`: the (N, H, W) float32 map, and under `..._raw` the raw map's (min, max) per layer and sample, (L, N, 2).  Arrays and names
only; parameters are NOT stored, both sides derive them from the seed (cls_oracle.seeded_params).  The shims (tests/gradcam_oracle.py; no reference file is
edited): `prob = 0.2` on the reference's ResNet modules (as tools/make_golden_cls.py), a stub `cv2` whose `resize` restates INTER_LINEAR (cv2 is not
installed; parity with cv2.resize itself is therefore NOT pinned), a stub `SimpleITK`, and a wrapper module that returns the (logits, softmax, argmax) triple
the class unpacks from `model(x)` - the reference's ResNet2d.forward returns the logits alone, so the class cannot run on it as shipped."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader        # noqa: E402
import gradcam_oracle as gco         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gradcam_2d.npz")


def main():
    if not ref_loader.available():
        sys.exit("reference tree not available; the golden can only be regenerated where it is")
    torch.set_num_threads(1)
    nets, GradCAM = gco.load_reference_gradcam()
    out = {"layer_sets": np.array(list(gco.LAYER_SETS)), "cases": np.array([c[0] for c in gco.CASES_2D])}
    for case in gco.CASES_2D:
        for ls, names in gco.LAYER_SETS.items():
            for cls in gco.golden_classes(case[3]):
                m, raw = gco.reference_maps(nets, GradCAM, case, names, cls)
                key = gco.golden_key(case[0], ls, cls)
                out[key], out[key + "_raw"] = m, raw
                print(key, m.shape, "map max per sample", m.reshape(m.shape[0], -1).max(1), "raw min/max", raw.reshape(-1, 2).tolist())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
