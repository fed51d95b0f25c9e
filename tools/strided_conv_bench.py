"""The stride-2 convolutions of the IR-SE backbone, per launch: the strided training entries (gim_conv2d_strided_fwd / _dgrad / _wgrad)
against what they replace - the stride-1 launch at full resolution plus the subsample pass (forward: conv + gim_subsample2_fwd;
input gradient: gim_subsample2_bwd + dgrad; weight gradient: wgrad on the zero-stuffed dy, whose gim_subsample2_bwd the dgrad column
already carries).  Timed through the C ABI with HIP events, the method of tools/conv_shapes_bench.py.

    python tools/strided_conv_bench.py [B=128] [reps=20] > strided_conv_shapes.txt
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from optimalstrategiesagainstgenerativeattacks_amd import _lib  # noqa: E402

# (H = W of the input, Cin, Cout, K): the four stride-2 3x3 convolutions of IR-SE-50 on 64x64 images, and its three convolution shortcuts
SHAPES = ((64, 64, 64, 3), (32, 128, 128, 3), (16, 256, 256, 3), (8, 512, 512, 3), (32, 64, 128, 1), (16, 128, 256, 1), (8, 256, 512, 1))


def time_ms(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    print("B = %d, %d repetitions after 3; ms per call; strided entry | what it replaces (stride-1 launch + subsample pass)" % (B, reps))
    print("%-22s %8s | %9s %9s %6s | %9s %9s %6s | %9s %9s %6s | %8s" % ("H,Cin,Cout,K", "GFLOP", "fwd", "old fwd", "x", "dgrad", "old dgrad", "x",
                                                                          "wgrad", "old wgrad", "x", "dgrad ks"))
    tot_new = tot_old = 0.0
    for S, Cin, Cout, K in SHAPES:
        Ho = S // 2
        x = torch.randn(B, S, S, Cin, device=dev)
        xs = torch.empty(B, Ho, Ho, Cin, device=dev)
        w = torch.randn(Cout, K, K, Cin, device=dev) * 0.05
        y, dy = torch.empty(B, Ho, Ho, Cout, device=dev), torch.randn(B, Ho, Ho, Cout, device=dev)
        y_full, dy_full = torch.empty(B, S, S, Cout, device=dev), torch.empty(B, S, S, Cout, device=dev)
        dx, dxs = torch.empty(B, S, S, Cin, device=dev), torch.empty(B, Ho, Ho, Cin, device=dev)
        acc = torch.zeros(Cout * K * K * Cin, device=dev)
        sh = _lib.GimInferConv(B, S, S, Cin, Cout, K, 2)
        p = lambda t: t.data_ptr()  # noqa: E731
        if K == 3:      # stride 1 at full resolution, then every other pixel
            full = _lib.GimConvShape(B, S, S, Cin, Cout, K, 0, 1.0, 0, 0, 0)

            def old_fwd():
                lib.gim_conv2d_fwd(p(x), p(w), None, None, None, p(y_full), full, st)
                lib.gim_subsample2_fwd(p(y_full), p(y), B, S, S, Cout, st)

            def old_dgrad():
                lib.gim_subsample2_bwd(p(dy), p(dy_full), B, S, S, Cout, st)
                lib.gim_conv2d_dgrad(p(dy_full), p(w), None, None, p(dx), full, st)

            def old_wgrad():
                lib.gim_conv2d_wgrad_acc(p(dy_full), p(x), p(acc), None, full, st)
        else:           # the 1x1 shortcut: the subsampled input through a stride-1 1x1 convolution
            half = _lib.GimConvShape(B, Ho, Ho, Cin, Cout, K, 0, 1.0, 0, 0, 0)

            def old_fwd():
                lib.gim_subsample2_fwd(p(x), p(xs), B, S, S, Cin, st)
                lib.gim_conv2d_fwd(p(xs), p(w), None, None, None, p(y), half, st)

            def old_dgrad():
                lib.gim_conv2d_dgrad(p(dy), p(w), None, None, p(dxs), half, st)
                lib.gim_subsample2_bwd(p(dxs), p(dx), B, S, S, Cin, st)

            def old_wgrad():
                lib.gim_conv2d_wgrad_acc(p(dy), p(xs), p(acc), None, half, st)
        old_fwd()
        old_dgrad()
        t = [time_ms(lambda: lib.gim_conv2d_strided_fwd(p(x), p(w), None, p(y), ctypes.byref(sh), st), reps), time_ms(old_fwd, reps),
             time_ms(lambda: lib.gim_conv2d_strided_dgrad(p(dy), p(w), p(dx), ctypes.byref(sh), 0, st), reps), time_ms(old_dgrad, reps),
             time_ms(lambda: lib.gim_conv2d_strided_wgrad(p(dy), p(x), p(acc), None, ctypes.byref(sh), 1, None, st), reps), time_ms(old_wgrad, reps)]
        plan = (ctypes.c_int32 * 16)()
        lib.gim_conv2d_strided_plan(ctypes.byref(sh), 1, ctypes.cast(plan, ctypes.c_void_p))
        ks = "/".join(str(plan[4 * i + 3]) for i in range(4))
        gf = 2.0 * B * Ho * Ho * Cin * Cout * K * K / 1e9
        print("%-22s %8.2f | %9.4f %9.4f %6.2f | %9.4f %9.4f %6.2f | %9.4f %9.4f %6.2f | %8s" %
              ("%d,%d,%d,%d" % (S, Cin, Cout, K), gf, t[0], t[1], t[1] / t[0], t[2], t[3], t[3] / t[2], t[4], t[5], t[5] / t[4], ks))
        tot_new += t[0] + t[2] + t[4]
        tot_old += t[1] + t[3] + t[5]
    print("sum over the seven convolutions, three directions: %.3f ms strided, %.3f ms stride-1 + subsample" % (tot_new, tot_old))


if __name__ == "__main__":
    main()
