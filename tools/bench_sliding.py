"""Sliding-window inference on one GPU: `inference_sliding` beside `inference_patch` on a synthetic 192 x 192 x 256 volume with a 96^3 patch,
and the achieved bytes/s of the three kernels of csrc/sliding.hip next to a device-to-device copy that moves the same number of bytes
(read + written), timed in the same process with device events.  Bytes are algorithmic, computed from the shapes: every input read once,
every output written once.  Prints JSON lines; asserts nothing."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pytorchdeeplearing_amd import prepost as PP

VOL, PATCH = (192, 192, 256), (96, 96, 96)
dev = torch.device("cuda:0")


def timed(fn, reps=50, warm=5):
    """mean milliseconds per call between two device events"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def copy_ms(nbytes):
    """a device-to-device copy that reads nbytes / 2 and writes nbytes / 2"""
    n = max(1, nbytes // 8)
    src, dst = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    return timed(lambda: dst.copy_(src))


def row(name, ms, nbytes):
    c = copy_ms(nbytes)
    print(json.dumps({"kernel": name, "ms": round(ms, 4), "algorithmic_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1),
                      "copy_same_bytes_ms": round(c, 4), "copy_GBps": round(nbytes / c / 1e6, 1), "kernel_over_copy": round(ms / c, 3)}), flush=True)


def kernels(c, nb):
    """nb = 4: one batch of the wrapper run below (for small C its working set stays in the 256 MiB Infinity Cache, so the rates are
    cache rates, like the copy's beside them); nb = 45: the whole window list in one batch, hundreds of MB per call.  The entry points
    are called directly with prepared pointers: a call through the prepost functions costs more host time than these kernels run."""
    from pytorchdeeplearing_amd import _capi
    lib, st = _capi.product_library(), _capi.stream_for(dev)
    torch.manual_seed(0)
    vol = torch.randn(VOL, device=dev)
    origins = PP.window_origins(VOL, PATCH, 0.5)[:nb]
    entries = torch.tensor([o + ((7 if i % 2 else 0),) for i, o in enumerate(origins)], dtype=torch.int32, device=dev)     # every other window mirrored
    pv, v = int(np.prod(PATCH)), int(np.prod(VOL))
    probs = torch.rand((nb, c) + PATCH, device=dev)
    batch = torch.empty((nb, 1) + PATCH, device=dev)
    w = [torch.from_numpy(PP.importance_1d(p, "gaussian")).to(dev) for p in PATCH]
    acc, wsum = torch.zeros((c,) + VOL, device=dev), torch.zeros(VOL, device=dev)
    mask, pout = torch.empty(VOL, dtype=torch.uint8, device=dev), torch.empty((c,) + VOL, device=dev)
    I3 = _capi.C.c_int * 3
    lo = I3(*(min(o[a] for o in origins) for a in range(3)))
    hi = I3(*(max(o[a] for o in origins) + PATCH[a] for a in range(3)))
    box = int(np.prod([h - l for l, h in zip(lo, hi)]))
    tag = "C=%d nb=%d" % (c, nb)
    row("gather_windows " + tag, timed(lambda: lib.seg_op_gather_windows(vol.data_ptr(), *VOL, entries.data_ptr(), nb, *PATCH, 0.0, batch.data_ptr(), st)),
        2 * 4 * nb * pv)
    row("blend_windows " + tag, timed(lambda: lib.seg_op_blend_windows(probs.data_ptr(), entries.data_ptr(), nb, c, *PATCH, w[0].data_ptr(), w[1].data_ptr(),
                                                                      w[2].data_ptr(), lo, hi, acc.data_ptr(), wsum.data_ptr(), *VOL, st)),
        4 * nb * c * pv + 2 * 4 * (c + 1) * box)
    row("blend_finalize " + tag, timed(lambda: lib.seg_op_blend_finalize(acc.data_ptr(), wsum.data_ptr(), c, v, 0.5, 1, mask.data_ptr(), None, st)),
        4 * (c + 1) * v + v)
    row("blend_finalize+probs " + tag, timed(lambda: lib.seg_op_blend_finalize(acc.data_ptr(), wsum.data_ptr(), c, v, 0.5, 1, mask.data_ptr(),
                                                                              pout.data_ptr(), st)), 4 * (2 * c + 1) * v + v)


def wrappers():
    import model
    os.environ.setdefault("SEGENGINE_DTYPE", "f16")
    ct = (-1024.0 + 224.0 * np.random.RandomState(1).rand(*VOL)).astype(np.float32)
    u = model.BinaryUNet3dModel(96, 96, 96, 1, 1, 4, use_cuda=True)
    kw = dict(newSpacing=(1.0, 1.0, 1.0), spacing=(1.0, 1.0, 1.0))
    runs = {
        "inference_patch (8 windows, OR of hard masks)": lambda: u.inference_patch(ct, **kw),
        "inference_sliding (45 windows in 12 batches, gaussian blend)": lambda: u.inference_sliding(ct, clip=(-1024.0, -800.0), **kw),
        "inference_sliding (45 windows x 2 mirrors in 23 batches)": lambda: u.inference_sliding(ct, clip=(-1024.0, -800.0), mirror_axes=(2,), **kw),
    }
    import time
    for name, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()                                    # ends in the device-to-host copy of the mask: synchronised
        ms = (time.perf_counter() - t0) / 3 * 1e3
        print(json.dumps({"op": "BinaryUNet3dModel.%s %dx%dx%d, patch 96^3, batch 4, f16, host array in / host mask out" % ((name,) + VOL),
                          "ms": round(ms, 2)}), flush=True)


if __name__ == "__main__":
    from pytorchdeeplearing_amd import _capi
    print(json.dumps({"build": _capi.product_library().build_info(), "device": torch.cuda.get_device_name(0)}), flush=True)
    for c, nb in ((1, 4), (3, 4), (16, 4), (1, 45), (3, 45), (16, 45)):
        kernels(c, nb)
    wrappers()
