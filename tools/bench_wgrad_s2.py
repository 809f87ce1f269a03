"""Op-level timing of the 2^d stride-2 weight gradients through the operator boundary (seg_op_wgrad = kernel + partial-tile reduce): wgrad_s2_kernel with its
own slices (SEG_WG_S2 unset), on wgrad_kernel's slices (=2) and wgrad_kernel (=0), on the layer shapes of VNet3d 4 x 96^3 and a few others.  One child
process per arm, arms alternating, one JSON line per child: {shape: [us, GB/s over both operands read once + the partial tiles written and read back,
slices]}.  An arm is a comma-separated list of environment settings, e.g. SEGENGINE_LIB=...,SEG_WG_S2=0 (tools/build_variant.py builds).

    python tools/bench_wgrad_s2.py [--rounds R] [arm ...]"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# role, ndim, N, coarse extents, P, Q
SHAPES = [("conv", 3, 4, (48, 48, 48), 32, 16), ("convT", 3, 4, (48, 48, 48), 32, 16), ("conv", 3, 1, (80, 80, 80), 32, 16),
          ("convT", 3, 2, (64, 64, 64), 32, 16), ("conv", 2, 16, (256, 256), 32, 16), ("convT", 3, 4, (48, 48, 48), 64, 16),
          ("conv", 3, 4, (24, 24, 24), 64, 32)]          # the last one: 48^3 -> 24^3, 32 -> 64 channels - not eligible, wgrad_kernel in every arm

if len(sys.argv) > 1 and sys.argv[1] == "child":
    import torch
    from pytorchdeeplearing_amd import _capi, ops
    dev = torch.device("cuda")
    lib = _capi.lib_for(dev)
    res = {"kernel": {}}
    for role, ndim, N, sp, P, Q in SHAPES:
        sp3 = sp if ndim == 3 else (1,) + sp
        fine = tuple(2 * s for s in sp) if ndim == 3 else (1,) + tuple(2 * s for s in sp)
        dr = ops.aligned_like(torch.randn((N,) + sp3 + (P,), device=dev).half())
        x = ops.aligned_like(torch.randn((N,) + fine + (Q,), device=dev).half())
        a = ops.WgradArgs()
        a.dr, a.x0, a.C0, a.x1, a.C1 = dr.data_ptr(), x.data_ptr(), Q, None, 0
        a.taps = ops.make_taps(ndim, 2, 0)
        T = a.taps.n
        a.P, a.Q, a.N = P, Q, N
        a.ID, a.IH, a.IW = fine
        a.OD, a.OH, a.OW = sp3
        a.sd, a.sh, a.sw = (2 if ndim == 3 else 1), 2, 2
        a.sP, a.sQ, a.sT, a.stem = Q * T, T, 1, 0
        dw = ops.aligned_like(torch.zeros(P * Q * T, device=dev))
        a.dw = dw.data_ptr()
        scratch = ops.aligned_empty(lib.seg_op_wgrad_partial_bytes(C.byref(a)), dev).view(torch.float32)
        scratch.fill_(float("nan"))
        fn = lambda: lib.check(lib.seg_op_wgrad(C.byref(a), scratch.data_ptr(), _capi.DTYPE["f16"], _capi.stream_for(dev)), "seg_op_wgrad")
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        used = int((~torch.isnan(scratch)).sum())          # floats of the partial tiles this launch writes
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            fn()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) / 20 * 1e3
        tag = "%s %dd N%d %s %d->%d" % (role, ndim, N, "x".join(map(str, sp)), *((Q, P) if role == "conv" else (P, Q)))
        res[tag] = [round(us, 1), round((dr.numel() * 2 + x.numel() * 2 + 2 * used * 4) / us * 1e-3, 1), used // (P * Q * T)]
        res["kernel"][tag] = lib.seg_op_wgrad_kernel(C.byref(a), _capi.DTYPE["f16"])
    print(json.dumps(res))
else:
    args = sys.argv[1:]
    rounds = 2
    if args and args[0] == "--rounds":
        rounds, args = int(args[1]), args[2:]
    arms = [a.split(",") for a in args] or [["SEG_WG_S2=0"], ["SEG_WG_S2=2"], ["SEG_WG_S2=1"]]
    for r in range(rounds):
        for arm in arms:
            env = dict(os.environ)
            env.update(dict(kv.split("=", 1) for kv in arm))
            out = subprocess.run([sys.executable, __file__, "child"], env=env, capture_output=True, text=True, timeout=300)
            line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else json.dumps({"error": out.stderr[-400:]})
            print(json.dumps({"round": r, "arm": " ".join(arm), "result": json.loads(line)}), flush=True)
            if out.returncode:
                sys.exit(out.returncode)          # a failed child ends the run: nothing more is started on the device
