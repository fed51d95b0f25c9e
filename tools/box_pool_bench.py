#!/usr/bin/env python
"""Per-layer A/B of the pooled 3x3 convolutions: the folded launch (gim_conv_shape.pool = 1, 16 taps on x) against the box pass
(gim_box2_fwd) plus the 9-tap launch on the box-filtered input (pool = 2), forward and weight gradient, isolated, through the C ABI
with device events.  The input gradient runs the folded launch on both routes and is not timed.

    python tools/box_pool_bench.py [--iters 50] [--out profiles/box_pool_per_layer.txt]

Each timing is the median over --iters back-to-back launches between two events after a warm-up of the same launches; the weight
gradient accumulates into a zeroed slot (gim_conv2d_wgrad_acc, the queued route of the training step).  GB/s of the box pass counts
one read of x and one write of p."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimalstrategiesagainstgenerativeattacks_amd import _lib, ops   # noqa: E402

# the pooled 3x3 layers of the vox64 step (conv_r2 of every ResBlockDown) at its three batch sizes: 16 episodes, 80- and 160-image sets
LAYERS = [(64, 64, 64, 64), (32, 32, 128, 128), (16, 16, 256, 256), (8, 8, 512, 512)]     # H, W, Cin, Cout
BATCHES = [16, 80, 160]


def timed(fn, iters, reps=7):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / iters)
    ts.sort()
    return ts[len(ts) // 2]


def tune(lib, st, dev, iters):
    """The sweep of tools/conv_autotune.py (tile x split-K for the forward, tile x slice target for the weight gradient) on the 9-tap
    launches, which that tool does not record (it keys by the ConvFn's folded geometry): prints rows for csrc/conv_tune_table.inc
    where a candidate beats the heuristic by > 3 %."""
    for N in BATCHES:
        for H, W, Cin, Cout in LAYERS:
            p = torch.randn(N, H + 1, W + 1, Cin, device=dev)
            w = torch.randn(Cout, 3, 3, Cin, device=dev) * 0.05
            y = torch.randn(N, H // 2, W // 2, Cout, device=dev)
            acc = torch.zeros(Cout * 9 * Cin, device=dev)
            M = N * (H // 2) * (W // 2)

            def shape(tile=-1, ks=0, tg=0):
                s = _lib.GimConvShape(N, H, W, Cin, Cout, 3, 0, 1.0, 2, 0, 0, tile, ks, tg)
                s.out_zeroed = 1
                return s
            runs = {"fwd": (lambda s: _lib.check(lib.gim_conv2d_fwd(p.data_ptr(), w.data_ptr(), None, None, None, y.data_ptr(), s, st)),
                            [(tl, ks, 0) for tl in ([128, 641, 1264, 64, 6432] if Cout > 64 else [1264, 64, 6432]) for ks in (1, 2, 3, 4, 6)],
                            (7, M, Cin, Cout, 9 * Cin, 0)),
                    "wgrad": (lambda s: _lib.check(lib.gim_conv2d_wgrad_acc(y.data_ptr(), p.data_ptr(), acc.data_ptr(), None, s, st)),
                              [(tl, 0, tg) for tl in (0, 128, 641, 1264, 64, 6432) for tg in (128, 256, 512, 1024, 2048, 4096)],
                              (2, M, Cout, 9 * Cin, 3, 4))}
            for kind, (fn, cands, key) in runs.items():
                s0 = shape()
                t_auto = timed(lambda: fn(s0), iters, reps=3)
                best = (t_auto, 0, 0)
                for tl, ks, tg in cands:
                    sc = shape(tl if tl else -1, ks, tg)
                    t = timed(lambda: fn(sc), iters, reps=3)
                    if t < best[0]:
                        best = (t, tl, ks if kind == "fwd" else tg)
                gain = t_auto / best[0] - 1.0
                row = "    {%d, %d, %d, %d, %d, %d, %d, %d},  // %s box %d,%d,%d,%d,%d: +%.0f %%" % (key + (best[1], best[2], kind, N, H, W, Cin, Cout, gain * 100))
                print("%-5s %-20s heuristic %7.1f us  best %7.1f us  %s" % (kind, "%d,%d,%d,%d,%d" % (N, H, W, Cin, Cout), t_auto, best[0],
                                                                          row if gain > 0.03 else "(heuristic stays)"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tune", action="store_true", help="sweep launch configurations of the 9-tap launches and print table rows")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    if a.tune:
        return tune(lib, st, dev, a.iters)
    lines = ["# pooled 3x3 convs, isolated, us per launch (median of 7 x %d launches): fold = pool-folded launch (16 taps);" % a.iters,
             "# box = gim_box2_fwd pass + 9-tap launch on the box-filtered input.  The wgrad reads the saved box map: no pass.",
             "%-22s | %8s %8s %8s %8s %7s | %8s %8s | %s" % ("N,H,W,Cin,Cout", "fwd fold", "box pass", "box conv", "box sum", "GB/s",
                                                             "wg fold", "wg box", "verdict (fwd / wgrad)")]
    for N in BATCHES:
        for H, W, Cin, Cout in LAYERS:
            x = torch.randn(N, H, W, Cin, device=dev)
            p = torch.empty(N, H + 1, W + 1, Cin, device=dev)
            w = torch.randn(Cout, 3, 3, Cin, device=dev) * 0.05
            wf = torch.randn(Cout, 4, 4, Cin, device=dev) * 0.05
            y = torch.randn(N, H // 2, W // 2, Cout, device=dev)
            acc = torch.zeros(Cout * 16 * Cin, device=dev)
            bacc = torch.zeros(Cout, device=dev)
            s_fold = ops._shape(N, H, W, Cin, Cout, 3, 0, 1.0, 1, 1, 0)
            s_box = ops._shape(N, H, W, Cin, Cout, 3, 0, 1.0, 2, 0, 0)
            for s in (s_fold, s_box):
                s.out_zeroed = 1      # (a split-K launch would add into y: timing only)
            chk = _lib.check
            t_ff = timed(lambda: chk(lib.gim_conv2d_fwd(x.data_ptr(), wf.data_ptr(), None, None, None, y.data_ptr(), s_fold, st)), a.iters)
            t_bp = timed(lambda: chk(lib.gim_box2_fwd(x.data_ptr(), p.data_ptr(), N, H, W, Cin, 0.2, st)), a.iters)
            t_bc = timed(lambda: chk(lib.gim_conv2d_fwd(p.data_ptr(), w.data_ptr(), None, None, None, y.data_ptr(), s_box, st)), a.iters)
            t_wf = timed(lambda: chk(lib.gim_conv2d_wgrad_acc(y.data_ptr(), x.data_ptr(), acc.data_ptr(), bacc.data_ptr(), s_fold, st)), a.iters)
            t_wb = timed(lambda: chk(lib.gim_conv2d_wgrad_acc(y.data_ptr(), p.data_ptr(), acc.data_ptr(), bacc.data_ptr(), s_box, st)), a.iters)
            gbs = (x.numel() + p.numel()) * 4 / (t_bp * 1e-6) / 1e9
            verdict = "%s / %s" % ("box" if t_bp + t_bc < t_ff else "FOLD", "box" if t_wb < t_wf else "FOLD")
            lines.append("%-22s | %8.1f %8.1f %8.1f %8.1f %7.0f | %8.1f %8.1f | %s" % (
                "%d,%d,%d,%d,%d" % (N, H, W, Cin, Cout), t_ff, t_bp, t_bc, t_bp + t_bc, gbs, t_wf, t_wb, verdict))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
