#!/usr/bin/env python3
"""Record what gim_conv_launch_plan answers, per shape, as tests/golden/launch_plans.json (tests/test_launch_plan_fixture.py).

Run it against a library built from the commit whose plans are the reference - NOT from the tree under test:

    git worktree add /tmp/base <commit> && make -C /tmp/base/optimalstrategiesagainstgenerativeattacks_amd/csrc
    GIM_LIB_PATH=/tmp/base/optimalstrategiesagainstgenerativeattacks_amd/csrc/libgim_hip.so \
        python tools/record_launch_plans.py --commit $(git rev-parse <commit>)

No GPU needed: the plan query launches nothing.  Corpus: every shape of the launch table (tests/test_gpu_tuned_rows.py::SHAPES)
plus a sweep over batch, map, channel pair, kernel size and the four (ups, pool, wfold) forms; each under the overrides below, on all
four plan kinds.  The full rows are several MB, so the fixture keeps a 12-hex-digit digest per shape.

With --strided the same for gim_conv2d_strided_plan (kinds 0, 1, 2) and gim_conv2d_strided_wgrad_workspace, over a sweep of its own:
tests/golden/strided_plans.json (tests/test_strided_plan_fixture.py).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OVERRIDES = [
    {},
    {"tune_ksplit": 1},
    {"prec": 1},
    {"tune_tile": -1},
    {"tune_tile": 64},
    {"tune_tile": 6432},
    {"tune_tile": 1264},
    {"tune_tile": 20128},
    {"tune_tile": 20641, "tune_ksplit": 3},
    {"tune_tile": 20000, "tune_wgrad": 512},
    {"tune_wgrad": 256},
    {"post_slope": 0.2},
    {"res_ups": 1},
]
BATCHES = (1, 16, 32, 80, 240)
MAPS = ((1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (64, 64), (8, 2), (2, 8))     # (H, W): the square maps and two narrow ones
CHANNELS = ((3, 64), (64, 3), (3, 3), (1, 1), (6, 64), (64, 64), (128, 256), (512, 512), (48, 40), (5120, 512))
KS = (1, 3, 9)
FORMS = ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 1, 1))      # (ups, pool, wfold)


def corpus():
    from tests.test_gpu_tuned_rows import SHAPES
    shapes = list(SHAPES)
    seen = set(shapes)
    for N in BATCHES:
        for H, W in MAPS:
            for Cin, Cout in CHANNELS:
                for K in KS:
                    for ups, pool, fold in FORMS:
                        cfg = (N, H, W, Cin, Cout, K, ups, 0.2, pool, fold)
                        if cfg not in seen:
                            seen.add(cfg)
                            shapes.append(cfg)
    return shapes


# gim_conv2d_strided_plan / gim_conv2d_strided_wgrad_workspace (--strided): batches up to halved-twice, maps from the smallest accepted
# to 256 x 256 with two narrow and two refused ones, aligned and generic channel pairs, a refused kernel size and a refused stride
S_BATCHES = (1, 2, 32, 128, 600, 4096)
S_MAPS = ((2, 2), (4, 4), (8, 8), (16, 16), (64, 64), (128, 128), (256, 256), (8, 2), (2, 8), (1, 1), (12, 8))
S_CHANNELS = ((16, 16), (64, 64), (64, 128), (128, 256), (256, 512), (512, 512), (3, 64), (48, 40), (8, 16))
S_KS = (1, 3, 5)
S_STRIDES = (1, 2, 3)


def strided_corpus():
    return [(N, H, W, Cin, Cout, K, st) for N in S_BATCHES for H, W in S_MAPS for Cin, Cout in S_CHANNELS for K in S_KS for st in S_STRIDES]


def record_strided(commit, out_path):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    from tests.test_launch_plan_fixture import rows_digest
    from tests.test_strided_plan_fixture import COUNTS, KINDS, count_into, shape_key, strided_rows
    lib = _lib.load()
    digests, counts = {}, dict.fromkeys(COUNTS, 0)
    for cfg in strided_corpus():
        rows = strided_rows(lib, cfg)
        count_into(counts, cfg, rows)
        digests[shape_key(cfg)] = rows_digest(rows)
    fx = {"parent_commit": commit, "kinds": list(KINDS), "counts": counts, "shapes": digests}
    with open(out_path, "w") as f:
        json.dump(fx, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d shapes x (%d plan kinds + workspace); %s -> %s (%d bytes)" % (len(digests), len(KINDS), counts, out_path, os.path.getsize(out_path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="full hash of the commit the loaded library was built from")
    ap.add_argument("--strided", action="store_true", help="record the strided queries (tests/golden/strided_plans.json) instead")
    ap.add_argument("--out", default=None, help="default: the fixture under tests/golden/")
    args = ap.parse_args()
    assert len(args.commit) == 40, "--commit: the full 40-digit hash"
    if args.strided:
        return record_strided(args.commit, args.out or os.path.join(ROOT, "tests", "golden", "strided_plans.json"))
    args.out = args.out or os.path.join(ROOT, "tests", "golden", "launch_plans.json")
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    from tests.test_launch_plan_fixture import KINDS, plan_rows, rows_digest, shape_key
    lib = _lib.load()
    digests, n_err, forms, n = {}, 0, {1: 0, 2: 0, 3: 0}, 0
    for cfg in corpus():
        rows = plan_rows(lib, cfg, OVERRIDES)
        n += len(rows)
        n_err += sum(1 for r in rows if r[2] != 0)
        for r in rows:
            if r[2] == 0 and (r[10] & 255) in forms:
                forms[r[10] & 255] += 1
        digests[shape_key(cfg)] = rows_digest(rows)
    fx = {"parent_commit": args.commit, "kinds": list(KINDS), "overrides": OVERRIDES, "argument_errors": n_err, "forms": forms, "shapes": digests}
    with open(args.out, "w") as f:
        json.dump(fx, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d shapes x %d overrides x %d kinds = %d plans; %d argument errors; forms (1 patch, 2 fp16, 3 tiny) %s -> %s (%d bytes)"
          % (len(digests), len(OVERRIDES), len(KINDS), n, n_err, forms, args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
