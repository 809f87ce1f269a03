"""Register-blocked halo conv (csrc/conv3x.hip) against torch.nn.functional on integer-valued data: every tiling of the
kernel (every row of the table in csrc/conv3x_impl.h, as the library enumerates it), forward (+ bias + GroupNorm partial sums),
data-gradient (flipped fragment-major weights), virtual concat inputs (aligned and straddling a 32-channel chunk), partial
boxes, several chunk groups; and the default tiling per layer shape against a recorded table.  Bit-exact for f16 and bf16."""
import functools
import json
import os

import pytest

import conftest
import torch
import torch.nn.functional as F

from pytorchdeeplearing_amd import ops
from pytorchdeeplearing_amd import _capi
from test_ops import cl, ncdhw, ints, to_dev

BF16_CHECKER_WORK = 3_000_000       # voxels x Cin x Cout x tilings above which a bf16 case is left to the GPU run (15-40 s on the host checker)

# ndim, N, spatial, Cin (list = concat sources), Cout, tiling ids to run (None: the default pick)
CASES = [
    (3, 1, (3, 9, 18), [32], 32, [0, 1, 13, 14, 20, 21, 22, 23]),          # partial boxes in every direction
    (3, 2, (2, 8, 16), [64], 64, [2, 15]),
    (3, 1, (4, 8, 10), [64], 64, [3, 4, 5, 6, 11]),
    (3, 1, (3, 5, 12), [128], 128, [7, 8, 9, 12]),
    (3, 1, (2, 4, 6), [256], 64, [11, 7]),                  # two chunk groups of four resident chunks
    (3, 1, (2, 8, 16), [32], 16, [10]),
    (3, 1, (2, 6, 16), [16, 16], 32, [0]),                  # concat straddling one 32-channel chunk
    (3, 1, (2, 5, 8), [32, 32], 64, [3]),                   # concat on a chunk boundary
    (3, 1, (2, 4, 8), [64, 64], 64, [None]),
    (3, 1, (3, 9, 18), [16], 16, [24, 25]),                 # Cin == 16: two taps per MFMA step, flat-K weights
    (3, 2, (2, 8, 32), [16], 32, [26, 27]),
    (3, 1, (3, 9, 18), [16], 16, [28, 29, None]),           # Cin == 16, halo fragments reused across the kh taps (weight layout 3); partial boxes
    (3, 2, (5, 8, 32), [16], 16, [29, None]),
    (2, 1, (19, 24), [16], 16, [56]),
    (2, 2, (16, 16), [16], 32, [57, None]),
    (2, 2, (17, 20), [32], 32, [32, 39]),
    (2, 1, (16, 32), [64], 64, [33, 34, 35, 38]),
    (2, 1, (9, 16), [128], 128, [36]),
    (2, 1, (8, 16), [32], 16, [37]),
    (2, 1, (12, 24), [16, 16], 64, [38]),
]


def check_forward(dev, dtype, ndim, cout, x0, x1, wf, b, ref, rs, cfg):
    """one forward launch of tiling `cfg` (None: the default pick): output and GroupNorm sum / sum of squares, bit for bit"""
    out, stats = ops.conv3x(x0, wf, dtype, ndim, cout, bias=ops.aligned_like(b.to(dev)), want_stats=True, x1=x1,
                            cfg=-1 if cfg is None else cfg)
    got = ncdhw(out.float().cpu(), ndim)
    assert torch.equal(got, ref), (cfg, float((got - ref).abs().max()))
    assert torch.equal(stats.cpu(), rs), cfg


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_conv3x_exact(dev, dtype, case):
    ndim, N, sp, cins, cout, cfgs = case
    cin = sum(cins)
    vox = N * sp[0] * sp[1] * (sp[2] if ndim == 3 else 1)
    if dtype == "bf16" and vox * cin * cout * len(cfgs) > BF16_CHECKER_WORK:       # bf16 arithmetic is the slow part of the host checker
        conftest.checker_slow(dev, "big bf16 case (the f16 twin runs here)")
    g = torch.Generator().manual_seed(sum(sp) * 3 + cin + cout)
    x = ints((N, cin) + sp, -2, 2, g)
    w = ints((cout, cin) + (3,) * ndim, -1, 1, g, density=0.1)
    b = ints((cout,), -3, 3, g)
    conv = F.conv3d if ndim == 3 else F.conv2d
    xr = x.clone().requires_grad_(True)
    ref = conv(xr, w, b, padding=1)
    assert float(ref.abs().max()) <= 256
    dy = ints(tuple(ref.shape), -1, 1, g, density=0.3)
    ref.backward(dy)
    assert float(xr.grad.abs().max()) <= 256
    xs = torch.split(x, cins, dim=1)
    x0 = to_dev(cl(xs[0]), dtype, dev)
    x1 = to_dev(cl(xs[1]), dtype, dev) if len(xs) > 1 else None
    wf = ops.pack(w.to(dev), "conv_fwd", dtype, frag="all")          # every layout of the shape; conv3x picks the one the tiling reads
    rs = torch.stack([ref.detach().double().flatten(2).sum(2), (ref.detach().double() ** 2).flatten(2).sum(2)], dim=2)
    known = {c["id"]: c for c in ops.conv3x_cfgs(dev)}
    for cfg in cfgs:
        if cfg is not None:
            assert cfg in known and known[cfg]["ndim"] == ndim and cout % known[cfg]["bn"] == 0, (cfg, known.get(cfg))
        check_forward(dev, dtype, ndim, cout, x0, x1, wf, b, ref.detach(), rs, cfg)
    # data-gradient: K = Cout (a multiple of 32, or 16), one launch per concat source with its own flipped weights
    if cout % 32 == 0 or cout == 16:
        dyd = to_dev(cl(dy), dtype, dev)
        c_lo = 0
        for ci in cins:
            if ci % 16:
                continue
            wd = ops.pack(w[:, c_lo:c_lo + ci].contiguous().to(dev), "conv_dgrad", dtype, frag="all")
            got = ops.conv3x(dyd, wd, dtype, ndim, ci)
            assert torch.equal(ncdhw(got.float().cpu(), ndim), xr.grad[:, c_lo:c_lo + ci]), ("dgrad", ci)
            c_lo += ci


def test_conv3x_rejects_what_it_cannot_run(dev):
    x = to_dev(torch.zeros(1, 2, 4, 8, 16), "f16", dev)
    w = to_dev(torch.zeros(16, 27 * 16), "f16", dev)
    x1 = to_dev(torch.zeros(1, 2, 4, 8, 8), "f16", dev)
    with pytest.raises(RuntimeError):
        ops.conv3x(x1, w, "f16", 3, 16, x1=x1)      # Cin = 16 as a concat of 8 + 8
    x = to_dev(torch.zeros(1, 2, 4, 8, 32), "f16", dev)
    w = to_dev(torch.zeros(32, 27 * 32), "f16", dev)
    with pytest.raises(RuntimeError):
        ops.conv3x(x, w, "f16", 3, 32, cfg=2)       # tiling 2 produces 64 output channels per workgroup
    with pytest.raises(RuntimeError):
        ops.conv3x(x, w, "f16", 3, 32, cfg=33)      # a 2-D tiling


# ---- every row of the table ---------------------------------------------------------------------------------------------
def table_rows():
    """The tilings as the library enumerates them (seg_op_conv3x_cfg_info), read when the tests are collected: from the gfx950 library where it is
    built (it is plain host data there, no device is touched), else from the host checker.  Both are compiled from the one table; the test compares
    its row with the library it then runs on."""
    if os.path.exists(_capi.LIB_PATH):
        return ops.conv3x_cfgs("cuda:0")
    conftest.emu_library()
    return ops.conv3x_cfgs("cpu")


def pytest_generate_tests(metafunc):
    if "row" in metafunc.fixturenames:
        rows = table_rows()
        metafunc.parametrize("row", rows, ids=["cfg%d" % r["id"] for r in rows])


@functools.lru_cache(maxsize=None)
def row_problem(ndim, sp, cin, cout):
    """integer-valued input, weights, bias and the torch result with its per-channel sum / sum of squares; shared by the dtypes and devices"""
    g = torch.Generator().manual_seed(sum(sp) * 3 + cin + cout)
    x = ints((1, cin) + sp, -2, 2, g)
    w = ints((cout, cin) + (3,) * ndim, -1, 1, g, density=0.1)
    b = ints((cout,), -3, 3, g)
    ref = (F.conv3d if ndim == 3 else F.conv2d)(x, w, b, padding=1)
    assert float(ref.abs().max()) <= 256
    rs = torch.stack([ref.double().flatten(2).sum(2), (ref.double() ** 2).flatten(2).sum(2)], dim=2)
    return x, w, b, ref, rs


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_conv3x_every_tiling(dev, dtype, row):
    """Each row of the tiling table on the smallest problem at which a wrong box, bn or nres shows: one sample, a partial box in every direction
    (spatial = box + (1, 1, 2)), Cin = one full group of resident chunks (32 * nres; 16 for the Cin == 16 kernels), Cout = bn, bias on."""
    assert row in ops.conv3x_cfgs(dev), row                      # the library under test carries the same row
    ndim, (td, th, tw) = row["ndim"], row["box"]
    assert (td == 1) == (ndim == 2), row
    sp = (td + 1, th + 1, tw + 2) if ndim == 3 else (th + 1, tw + 2)
    frag = _capi.lib_for(dev).dll.seg_op_conv3x_cfg_frag(row["id"])
    assert frag in (1, 2, 3), row
    cin, cout = (32 * row["nres"] if frag == 1 else 16), row["bn"]
    vox = sp[0] * sp[1] * (sp[2] if ndim == 3 else 1)
    if dtype == "bf16" and vox * cin * cout > BF16_CHECKER_WORK:
        conftest.checker_slow(dev, "big bf16 case (the f16 twin runs here)")
    x, w, b, ref, rs = row_problem(ndim, sp, cin, cout)
    wf = ops.pack(w.to(dev), "conv_fwd", dtype, frag="all")
    check_forward(dev, dtype, ndim, cout, to_dev(cl(x), dtype, dev), None, wf, b, ref, rs, row["id"])


# ---- the default tiling per shape -----------------------------------------------------------------------------------------
def test_conv3x_default_cfg_is_pinned(dev):
    """tests/golden/conv3x_default_cfg.json: seg_op_conv3x_default_cfg over every halo-conv layer shape (forward and data-gradient) of the BASELINE
    configs C2 - C5 and over shapes on both sides of every branch of conv3x_pick (csrc/conv3x.hip), recorded on the host checker from the build of
    commit 0615676, the last one with the hand-written host copy of the tilings and the literal 2 x 4 x 12 box in the picker.  The function is host arithmetic, so
    the checker and the device share one table.  A change that moves a default on purpose re-records the "cfg" fields from its own build (the same call
    over the file's "shape" lists, f16) and says in its description which shapes moved and why."""
    with open(os.path.join(conftest.GOLDEN, "conv3x_default_cfg.json")) as f:
        golden = json.load(f)
    lib = _capi.lib_for(dev)
    assert len(golden["shapes"]) >= 80
    for rec in golden["shapes"]:
        got = lib.dll.seg_op_conv3x_default_cfg(*rec["shape"], _capi.DTYPE["f16"])
        assert got == rec["cfg"], (rec, got)
