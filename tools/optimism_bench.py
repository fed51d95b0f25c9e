"""What does the optimistic step cost?  Two measurements on one MI355X, both at the default workload (64x64x3, m1 n5 k10), in the
manner of tools/average_bench.py, whose timing loops this tool uses.

  kernels  gim_adam_optimism (16 bytes read + 8 written per element; its record-only form, omega = 0: 8 + 4) at the two bucket sizes
           of the workload, with adam_kernel (gim_adam_step, 28 bytes per element, the same access pattern) as the yardstick in the
           same run: device events around L launches after warm-up, rotating over buffer sets that together exceed the 256 MiB
           Infinity Cache twice over, repeated R times.
  steps    gim_step with the optimistic step off and on for both agents: two trainers in one process, timed in alternating rounds
           (wall clock between two device synchronisations, K steps after W warm-up steps per round).

    python tools/optimism_bench.py kernels
    python tools/optimism_bench.py steps

Prints a table; --json adds one JSON line."""
import argparse
import gc
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from average_bench import COPY_RATE, L3_BYTES, bucket_sizes, time_launches  # noqa: E402
from bench import build_trainer, synthetic_batch  # noqa: E402


def kernels(args, device):
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for agent, n in bucket_sizes(args, device).items():
        seg = torch.tensor([n], dtype=torch.int64, device=device)
        lr = torch.full((1,), 1e-4, device=device)
        for kernel, bytes_per, omega in (("adam_kernel", 28, None), ("gim_adam_optimism", 24, args.omega), ("gim_adam_optimism record", 12, 0.0)):
            n_sets = max(2, math.ceil(2 * L3_BYTES / (4 * 4 * n)) + 1)
            # p, g or prev, m, v: the moments stay as they are set here under the correction, and positive under Adam
            sets = [[torch.randn(n, device=device) * 0.05 for _ in range(3)] + [torch.full((n,), 1e-4, device=device)] for _ in range(n_sets)]
            step = torch.full((1,), 0 if omega is None else 1000, dtype=torch.int32, device=device)
            if omega is None:
                def launch(i):
                    p, g, m, v = sets[i]
                    _lib.check(lib.gim_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, seg.data_ptr(), lr.data_ptr(), 1,
                                                 0.0, 0.99, 1e-8, 1.0, step.data_ptr(), st))
            else:
                def launch(i, omega=omega):
                    p, prev, m, v = sets[i]
                    _lib.check(lib.gim_adam_optimism(p.data_ptr(), prev.data_ptr(), m.data_ptr(), v.data_ptr(), n, seg.data_ptr(),
                                                     lr.data_ptr(), 1, 0.0, 0.99, 1e-8, omega, step.data_ptr(), None, st))
            us = time_launches(launch, n_sets, args.launches, args.warmup, args.repeats)
            mean = sum(us) / len(us)
            rate = bytes_per * n / (mean * 1e-6)
            rows.append({"bucket": agent, "elements": n, "kernel": kernel, "bytes_per_element": bytes_per, "buffer_sets": n_sets,
                         "us": [round(u, 2) for u in us], "us_mean": round(mean, 2), "spread_us": round(max(us) - min(us), 2),
                         "tb_per_s": round(rate / 1e12, 3), "share_of_copy_rate": round(rate / COPY_RATE, 3)})
            del sets
            torch.cuda.empty_cache()
    for r in rows:
        adam = [a for a in rows if a["bucket"] == r["bucket"] and a["kernel"] == "adam_kernel"][0]
        r["rate_over_adam_kernel"] = round(r["tb_per_s"] / adam["tb_per_s"], 3)
    print("kernels: %d launches after %d warm-up launches per timed loop, %d loops; rotating buffer sets (more than 2 x 256 MiB in all)"
          % (args.launches, args.warmup, args.repeats))
    print("(the adam_kernel rows include its 1-thread counter kernel: gim_adam_step is two launches)")
    print("%-14s %10s  %-25s %4s %5s  %-28s %9s %9s %7s %6s %7s" % ("bucket", "elements", "kernel", "B/el", "sets", "us per launch, each loop",
                                                                    "mean us", "spread us", "TB/s", "share", "/ adam"))
    for r in rows:
        print("%-14s %10d  %-25s %4d %5d  %-28s %9.2f %9.2f %7.3f %6.3f %7.3f"
              % (r["bucket"], r["elements"], r["kernel"], r["bytes_per_element"], r["buffer_sets"], " ".join("%.2f" % u for u in r["us"]),
                 r["us_mean"], r["spread_us"], r["tb_per_s"], r["share_of_copy_rate"], r["rate_over_adam_kernel"]))
    return rows


def steps(args, device):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    leaked, real, si = synthetic_batch(args.batch, args.m, args.n, args.k, args.channels, args.size, device, 1234)
    runs = []
    for name, omega in (("off", None), ("both", args.omega)):
        G, tr = build_trainer(args.size, args.channels, args.n, args.m, args.k, device)
        if omega is not None:
            tr.impersonator_opt.enable_optimism(omega)
            tr.authenticator_opt.enable_optimism(omega)
        runs.append((name, G, tr, G.DataParallelMock(tr)))

    def timed(G, tr, trainer):
        def one():
            tr.do_global_step()
            tr.update_learning_rate()
            G.gim_step(trainer, leaked, real, si, defer_join=True)
        for _ in range(args.warmup):
            one()
        ops.join_lanes()
        torch.cuda.synchronize()
        gc.collect()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one()
        ops.join_lanes()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3
    res = {name: [] for name, _, _, _ in runs}
    for _ in range(args.rounds):
        for name, G, tr, trainer in runs:
            res[name].append(round(timed(G, tr, trainer), 3))
    print("steps: gim_step, %d episodes, %d steps after %d warm-up steps per round, %d alternating rounds, omega %g; ms_per_step"
          % (args.batch, args.steps, args.warmup, args.rounds, args.omega))
    for name, ms in res.items():
        print("  optimism %-5s %s   mean %.3f  spread %.3f" % (name, "  ".join("%.3f" % v for v in ms), sum(ms) / len(ms), max(ms) - min(ms)))
    off = sum(res["off"]) / len(res["off"])
    print("  both - off: %+.3f ms (per round: %s)" % (sum(res["both"]) / len(res["both"]) - off,
                                                      " ".join("%+.3f" % (a - b) for a, b in zip(res["both"], res["off"]))))
    tr = runs[1][2]
    print("  extra device memory (flat_prev): %.1f MB" % ((tr.impersonator_opt.flat_p.numel() + tr.authenticator_opt.flat_p.numel()) * 4 / 1e6))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "steps"])
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--m", type=int, default=1)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--omega", type=float, default=1.0)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    out = kernels(args, device) if args.what == "kernels" else steps(args, device)
    if args.json:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
