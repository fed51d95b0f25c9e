"""gim_conv2d_strided_plan and gim_conv2d_strided_wgrad_workspace answer what the recorded parent commit answered.

``tests/golden/strided_plans.json`` was written by ``tools/record_launch_plans.py`` from the library of the commit named in its
header, BEFORE the conv entry points came to share one batch halving, one fill per call and one gim_infer_conv validation.  Same rule
as tests/test_launch_plan_fixture.py: the fixture is never regenerated from the code under test.

Per shape the fixture holds a short digest over the return code and out[16] of the plan query for kinds 0, 1 and 2 and the return code
and byte count of the workspace query - argument errors included: they are part of the record.
"""
import ctypes
import json
import os

from tests.test_launch_plan_fixture import rows_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "strided_plans.json")
KINDS = (0, 1, 2)         # gim_conv2d_strided_fwd, _dgrad, _wgrad (atomic combine)
BUF_MAX_BYTES = 0x7FFFFFF0
COUNTS = ("halved", "k_sliced", "tapless", "argument_errors")


def shape_key(cfg):
    return ",".join(str(v) for v in cfg)


def strided_rows(lib, cfg):
    """[[kind, return code, out[0..15]] for the three plan kinds] + [[3, return code, bytes]] of cfg = (N, H, W, Cin, Cout, KH, stride);
    the outputs start from -2 / -1, so what a refused call leaves untouched is the same in every run."""
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    sh = _lib.GimInferConv(*cfg)
    out = (ctypes.c_int32 * 16)()
    rows = []
    for kind in KINDS:
        out[:] = [-2] * 16
        rc = lib.gim_conv2d_strided_plan(ctypes.byref(sh), kind, ctypes.cast(out, ctypes.c_void_p))
        rows.append([kind, rc] + list(out))
    nbytes = ctypes.c_int64(-1)
    rc = lib.gim_conv2d_strided_wgrad_workspace(ctypes.byref(sh), ctypes.byref(nbytes))
    rows.append([3, rc, nbytes.value])
    return rows


def count_into(counts, cfg, rows):
    """What the corpus must keep reaching: accepted shapes whose batch is halved, launches with more than one K (or pixel) slice,
    dgrad classes without taps, argument errors."""
    N, H, W, Cin, Cout, KH, stride = cfg
    plans = rows[:3]
    if rows[3][1] == 0 and stride in (1, 2) and N > 1 and 4 * N * max(H * W * Cin, (H // stride) * (W // stride) * Cout) > BUF_MAX_BYTES:
        counts["halved"] += 1
    for r in plans:
        if r[1] != 0:
            continue
        launches = [r[2 + 4 * i:6 + 4 * i] for i in range(4)]
        counts["k_sliced"] += sum(1 for l in launches if l[3] > 1)
        counts["tapless"] += sum(1 for l in launches if l == [0, 0, 0, 0])
    counts["argument_errors"] += sum(1 for r in rows if r[1] != 0)


def test_strided_plans_equal_the_recorded_parent():
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    fx = json.load(open(FIXTURE))
    shapes = fx["shapes"]
    assert len(fx["parent_commit"]) == 40 and fx["kinds"] == list(KINDS)
    assert len(shapes) >= 5000
    bad = []
    counts = dict.fromkeys(COUNTS, 0)
    for key, want in shapes.items():
        cfg = tuple(int(t) for t in key.split(","))
        rows = strided_rows(lib, cfg)
        count_into(counts, cfg, rows)
        if rows_digest(rows) != want:
            bad.append((key, rows))
    for key, rows in bad[:5]:
        print("shape %s: digest differs from the parent's; current rows [kind, rc, out[16] | bytes]:" % key)
        for r in rows:
            print("   ", r)
    assert not bad, "%d of %d shapes answer differently from commit %s: %s" % (len(bad), len(shapes), fx["parent_commit"][:7], [b[0] for b in bad[:20]])
    # the corpus reaches halved batches, split launches, tap-less classes and the argument errors (counts of the record, so that a
    # corpus that lost one of them is noticed)
    assert counts == fx["counts"], (counts, fx["counts"])
    assert all(counts[k] > 0 for k in COUNTS), counts
