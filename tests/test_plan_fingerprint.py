"""Pin of what the planner schedules: workspace size, fork events of a backward pass and, per kernel class, the launches of one forward + loss + backward with
the bytes / flops the schedule accounts for them.  The planner (csrc/engine_plan.hip) decides all of these on the host, so a refactor of it must leave every
figure EXACTLY as it was; times are not compared."""
import json
import os

import pytest

import conftest
from pytorchdeeplearing_amd import _capi
from test_engine import build, run_engine

GOLDEN = os.path.join(conftest.GOLDEN, "plan_fingerprint.json")
PLAN_KNOBS = ("SEG_GN_FOLD", "SEG_VHEAD", "SEG_STEMX", "SEG_CONV3X", "SEG_DUAL_GN", "SEG_RQ_FUSE", "SEG_HEAD_FUSE", "SEG_VACT", "SEG_GN_COOP")
# the smallest shapes the engine plans; together: fused and unfused stem, activation on load + sums on the data-gradient launch, head inside the activation
# pass, folded finalize, dual GroupNorm backward, the small-tensor group path, pool, the plain ConvTranspose
RUNS = {
    "vnet2d_s-f16-default": ("vnet2d_s", "f16", {}),
    "vnet2d_s-f16-vact2": ("vnet2d_s", "f16", {"SEG_VACT": "2"}),
    "vnet2d_s-f16-knobs_off": ("vnet2d_s", "f16", {k: "0" for k in PLAN_KNOBS}),
    "unet2d_s-f32-default": ("unet2d_s", "f32", {}),
    "unet2d_s-f32-knobs_off": ("unet2d_s", "f32", {k: "0" for k in PLAN_KNOBS}),
}


def fingerprint(run, dev, setenv, delenv):
    """-> (fingerprint, outputs of run_engine) of one forward + loss + backward with given masks; the knobs are read when the engine is created"""
    tag, dtype, knobs = RUNS[run]
    for k in PLAN_KNOBS:
        delenv(k, raising=False)
    for k, v in knobs.items():
        setenv(k, v)
    e, params, x, y, masks, alpha, loss = build(tag, dtype, dev, True)
    e.profile_enable(_capi.KERNEL_CLASSES)
    out = run_engine(e, x, y, masks, alpha, loss, dev)
    prof = e.profile_read()
    fp = {"workspace_bytes": int(e.lib.seg_workspace_bytes(e.h)), "fork_events": int(e.lib.seg_plan_count(e.h, 2)),
          "classes": {k: [v["calls"], v["bytes"], v["flops"]] for k, v in sorted(prof.items())}}
    return fp, out


@pytest.mark.parametrize("run", list(RUNS))
def test_plan_fingerprint(dev, run, monkeypatch):
    """tests/golden/plan_fingerprint.json was recorded on the host checker from the build of the commit BEFORE the planner was split into named parts.  Every
    figure is host arithmetic over the planned shapes (no kernel result enters), so the checker and the device share one table.  A change that alters the
    schedule on purpose regenerates it from its own build:
        python -c "import json, pytest, sys; sys.path.insert(0, 'tests'); import conftest, test_plan_fingerprint as t; mp = pytest.MonkeyPatch(); conftest.emu_library(); \
                   import torch; print(json.dumps({r: t.fingerprint(r, torch.device('cpu'), mp.setenv, mp.delenv)[0] for r in t.RUNS}, indent=1))"
    (torch.device('cuda:0') on the GPU) and says in its description which figures moved and why."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    want = golden[run]
    got, _ = fingerprint(run, dev, monkeypatch.setenv, monkeypatch.delenv)
    print(run, dev.type, json.dumps(got))
    assert got["workspace_bytes"] == want["workspace_bytes"]
    assert got["fork_events"] == want["fork_events"]
    assert got["classes"] == want["classes"]          # per class: [calls, bytes, flops], exact (doubles computed by the same host arithmetic)
