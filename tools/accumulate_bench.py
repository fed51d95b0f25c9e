"""What does gradient accumulation cost?  One accumulated gim_step on B episodes (micro_batches = A) against A plain gim_steps on
B / A episodes each - the same forward and backward work; the accumulated step saves A - 1 Adam updates and A - 1 sets of
spectral-norm power iterations.  Both are timed in alternating rounds inside one process (K steps after W warm-up steps per round,
wall clock between two device synchronisations), and the peak of torch's allocator over each timed region is recorded.

Public API only, and the keyword is omitted when A = 1: `--micro-batches 1` runs on a commit that does not have the feature.

    python tools/accumulate_bench.py --batch 16 --micro-batches 2                       # bench workload, 2 x 8
    python tools/accumulate_bench.py --batch 16 --micro-batches 4
    python tools/accumulate_bench.py --size 128 --m 5 --n 20 --k 20 --batch 8 --micro-batches 4 --steps 2 --warmup 1 --rounds 1 --no-plain
    python tools/accumulate_bench.py --size 128 --m 5 --n 20 --k 20 --batch 2 --micro-batches 1 --steps 2 --warmup 1 --rounds 1

Prints one JSON line."""
import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_trainer, synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16, help="episodes per optimizer step of the accumulated run")
    ap.add_argument("--micro-batches", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reg-param", type=float, default=0.0)
    ap.add_argument("--matrix-path", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--no-plain", action="store_true", help="time the accumulated step only")
    args = ap.parse_args()
    A, B = args.micro_batches, args.batch
    assert A >= 1 and B % A == 0
    device = torch.device("cuda", 0)
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    ops.set_matrix_path(args.matrix_path)
    leaked, real, si = synthetic_batch(B, args.m, args.n, args.k, args.channels, args.size, device, 1234)
    per = B // A

    def make():
        G, tr = build_trainer(args.size, args.channels, args.n, args.m, args.k, device, reg_param=args.reg_param)
        return G, tr, G.DataParallelMock(tr)

    def accumulated(G, tr, trainer):
        kw = {"micro_batches": A} if A > 1 else {}
        tr.do_global_step()
        tr.update_learning_rate()
        G.gim_step(trainer, leaked, real, si, defer_join=True, **kw)

    def plain(G, tr, trainer):
        for j in range(A):
            sl = slice(j * per, (j + 1) * per)
            tr.do_global_step()
            tr.update_learning_rate()
            G.gim_step(trainer, leaked[sl], real[sl], si[sl], defer_join=True)

    def timed(fn, state):
        for _ in range(args.warmup):
            fn(*state)
        ops.join_lanes()
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn(*state)
        ops.join_lanes()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20

    runs = [("accumulated", accumulated, make())]
    if not args.no_plain and A > 1:
        runs.append(("plain", plain, make()))
    res = {name: {"ms": [], "peak_mib": []} for name, _, _ in runs}
    for _ in range(args.rounds):
        for name, fn, state in runs:
            ms, peak = timed(fn, state)
            res[name]["ms"].append(round(ms, 3))
            res[name]["peak_mib"].append(round(peak, 1))
    out = {"workload": "%dx%dx%d m%d n%d k%d" % (args.size, args.size, args.channels, args.m, args.n, args.k), "episodes_per_update": B,
           "micro_batches": A, "steps": args.steps, "warmup": args.warmup, "matrix_path": args.matrix_path, "reg_param": args.reg_param,
           "accumulated_step_ms": res["accumulated"]["ms"], "accumulated_peak_mib": res["accumulated"]["peak_mib"]}
    if "plain" in res:
        out["plain_steps_ms"] = res["plain"]["ms"]          # A plain steps of B / A episodes
        out["plain_peak_mib"] = res["plain"]["peak_mib"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
