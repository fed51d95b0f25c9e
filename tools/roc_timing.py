"""Time of authentication_eval.roc_statistics on CUDA scores next to the host roc_auc on the same scores (DESIGN.md section 10,
"Calibrating a baseline's threshold").  One MI355X; host clock around calls that end in the record's host read, and device events
around the two launches alone.

    python tools/roc_timing.py [--n 100000] [--rounds 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optimalstrategiesagainstgenerativeattacks_amd import authentication_eval as ae  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000, help="scores per side")
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    for name, step in (("continuous", 0.0), ("ties (steps of 1/16)", 0.0625)):
        pos, neg = (rng.randn(a.n) + 0.5).astype(np.float32), (rng.randn(a.n) - 0.5).astype(np.float32)
        if step:
            pos, neg = (np.round(pos / step) * step).astype(np.float32), (np.round(neg / step) * step).astype(np.float32)
        gp, gn = torch.from_numpy(pos).to(dev), torch.from_numpy(neg).to(dev)
        for _ in range(3):
            stats = ae.roc_statistics(gp, gn)
        wall, launches = [], []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = ae.roc_statistics(gp, gn)
            wall.append(time.perf_counter() - t0)
        counts = torch.empty(3 * 2 * a.n, device=dev, dtype=torch.int32)
        record = torch.empty(ops.ROC_WORDS, device=dev, dtype=torch.int64)
        lib = ops._lib.load()
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.check(lib.gim_roc_calibrate(ops._p(gp), a.n, ops._p(gn), a.n, counts.data_ptr(), record.data_ptr(), ops._stream()), "roc")
            e1.record()
            torch.cuda.synchronize()
            launches.append(e0.elapsed_time(e1) * 1e-3)
        y_true = np.concatenate([np.ones(a.n), np.zeros(a.n)])
        y_score = np.concatenate([pos, neg])
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            auc = ae.roc_auc(y_true, y_score)
            host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_stats = ae.roc_statistics_host(pos, neg)
        t_host_stats = time.perf_counter() - t0
        assert stats == host_stats and stats["auc"] == auc
        pairs = (2.0 * a.n) * (2.0 * a.n)
        print("%s, %d + %d scores: roc_statistics on CUDA %.3f ms (median of %d, min %.3f; fill + counts + finish launches alone %.3f ms = "
              "%.2e candidate-score pairs / s); host roc_auc %.1f ms (median of 3, min %.1f); roc_statistics_host %.1f ms; auc %.6f, same dict"
              % (name, a.n, a.n, statistics.median(wall) * 1e3, a.rounds, min(wall) * 1e3, statistics.median(launches) * 1e3,
                 pairs / statistics.median(launches), statistics.median(host) * 1e3, min(host) * 1e3, t_host_stats * 1e3, auc), flush=True)


if __name__ == "__main__":
    main()
