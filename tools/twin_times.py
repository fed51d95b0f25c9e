"""Device-event times of the entry points whose per-call and batched / grouped forms share one device body (csrc/spectral.hip,
gemm.hip, the fold of conv_igemm.hip), at one benchmark-sized layer (Cout = Cin = 512, 3 x 3) and the attention shape (256 tokens,
K = 16, 16 images).  One MI355X; events around each call, median / min / max over the rounds.  To compare two builds, run it once per
library in alternating processes:

    GIM_LIB_PATH=/path/to/old/libgim_hip.so python tools/twin_times.py [--rounds 30]
    python tools/twin_times.py [--rounds 30]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optimalstrategiesagainstgenerativeattacks_amd import _lib as L  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd import ops  # noqa: E402

COUT, CIN, K = 512, 512, 3
T_TOK, T_K, T_B = 256, 16, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    p = lambda t: t.data_ptr() if t is not None else None
    n, nf, Kc = COUT * CIN * K * K, COUT * CIN * (K + 1) ** 2, CIN * K * K
    w = rnd(n) / np.sqrt(Kc)
    u, v = torch.nn.functional.normalize(rnd(COUT), dim=0), torch.nn.functional.normalize(rnd(Kc), dim=0)
    sigma = torch.tensor([1.7], device=dev)
    cases = []

    # per-call entries
    sn_out = [torch.empty(1, device=dev), torch.empty(COUT, device=dev), torch.empty(Kc, device=dev), torch.empty(9 * Kc + COUT, device=dev)]
    u1, v1 = u.clone(), v.clone()
    cases.append(("gim_spectral_sigma, training round", lambda: lib.gim_spectral_sigma(
        p(w), p(u1), p(v1), p(sn_out[0]), p(sn_out[1]), p(sn_out[2]), p(sn_out[3]), COUT, CIN, K, 1, st)))
    slabs, dw, scratch = rnd(2 * nf), torch.empty(n, device=dev), torch.empty(512 + nf, device=dev)
    for fold in (0, 1, 2):
        for sn in (0, 1):
            cases.append(("gim_wgrad_finish, 2 slabs, fold %d, %s" % (fold, "sigma" if sn else "plain"),
                          lambda fold=fold, sn=sn: lib.gim_wgrad_finish(p(slabs), None, 2, p(w) if sn else None, p(sigma) if sn else None,
                                                                        p(u) if sn else None, p(v) if sn else None, p(dw), None, p(scratch),
                                                                        COUT, CIN, K, fold, None, None, st)))
    f = torch.empty(nf, device=dev)
    cases.append(("gim_conv2d_fold_weights", lambda: lib.gim_conv2d_fold_weights(p(w), p(f), COUT, CIN, K, st)))

    # attention products: energy = f^T g (both k-contiguous), and the three other stride combinations of the same sizes
    fa, gb, e = rnd(T_B * T_TOK * T_K + 4), rnd(T_B * T_TOK * T_K), torch.empty(T_B * T_TOK * T_TOK, device=dev)
    strides = {"A k, B k": (T_K, 1, 1, T_K), "A k, B j": (T_K, 1, T_TOK, 1), "A i, B k": (1, T_TOK, 1, T_K), "A i, B j": (1, T_TOK, T_TOK, 1)}
    for name, (sAi, sAk, sBk, sBj) in strides.items():
        for off, kind in ((0, "vector"), (1, "scalar")):
            cases.append(("gim_bgemm %d x %d x %d x %d, %s, %s kernel" % (T_B, T_TOK, T_TOK, T_K, name, kind),
                          lambda off=off, s=(sAi, sAk, sBk, sBj): lib.gim_bgemm(p(fa) + 4 * off, p(gb), p(e), T_B, T_TOK, T_TOK, T_K, T_TOK * T_K,
                                                                                s[0], s[1], T_TOK * T_K, s[2], s[3], st)))

    # batched / grouped entries: the same layer as one-job tables
    fj = (L.GimFoldJob * 1)()
    fj[0] = (p(w), p(f), COUT, CIN, K, 0)
    ftab = [(0, c) for c in range((nf + 65535) // 65536)]
    ft = ops._DeviceTable(fj, ftab)
    cases.append(("gim_conv2d_fold_weights_batched, one job", lambda: lib.gim_conv2d_fold_weights_batched(ft.ptrs[0], ft.ptrs[1], len(ftab), st)))
    sj = (L.GimSnJob * 1)()
    base, u2, v2 = torch.empty(1 + COUT + Kc + 10 * Kc + COUT, device=dev), u.clone(), v.clone()
    sj[0] = (p(w), p(u2), p(v2), 0, 1, 1 + COUT, 1 + COUT + Kc, COUT, CIN, K, 0)
    R = min(8, (COUT + 63) // 64)
    per = (COUT + R - 1) // R
    scols = [(0, xb, r, per) for xb in range((Kc + 255) // 256) for r in range(R)]
    srows = [(0, rb) for rb in range((COUT + 3) // 4)]
    stab = ops._DeviceTable(sj, scols, srows)
    cases.append(("gim_spectral_sigma_batched, one job, training round", lambda: lib.gim_spectral_sigma_batched(
        stab.ptrs[0], 1, stab.ptrs[1], len(scols), stab.ptrs[2], len(srows), p(base), 1, st)))
    keep = []
    for label, folds, exclusive in (("fold 0 / 1 / 2, sigma, exclusive", (0, 1, 2), 1), ("fold 0 twice into one gradient, sigma", (0, 0), 0),
                                    ("fold 0 / 1, plain, exclusive", (0, 1), 1)):
        plain = "plain" in label
        wj = (L.GimWgradJob * len(folds))()
        wtab, shared = [], torch.zeros(n, device=dev)
        chunks = (n + 4095) // 4096
        for j, fold in enumerate(folds):
            src, tmp, part = rnd(nf if fold else n), torch.empty(n, device=dev), torch.empty(chunks, device=dev)
            grad = torch.zeros(n, device=dev) if exclusive else shared
            gb_ = torch.zeros(COUT, device=dev)
            keep.extend([src, tmp, part, grad, gb_])
            wj[j] = (p(src), None, None if plain else p(w), None if plain else p(sigma), None if plain else p(u), None if plain else p(v),
                     p(tmp), p(part), p(grad), p(gb_), COUT, CIN, K, fold, chunks, exclusive)
            wtab += [(j, c) for c in range(chunks)]
        wt = ops._DeviceTable(wj, wtab, [] if plain else wtab)
        keep.append(wt)
        cases.append(("gim_wgrad_finish_batched, " + label, lambda wt=wt, nb=len(wtab), nj=len(folds), plain=plain: lib.gim_wgrad_finish_batched(
            wt.ptrs[0], nj, wt.ptrs[1], nb, wt.ptrs[2], 0 if plain else nb, st)))
    M, N, KK = 80, 512, 512      # style projections: nn.Linear(512, C) on one style matrix
    A, B, C = rnd(M * KK), rnd(N * KK), torch.zeros(M * N, device=dev)
    gj = (L.GimGemmJob * 4)()
    gt = []
    for j in range(4):
        gj[j] = (p(A), p(B), p(C), None, M, N, KK, N, KK, 1, 1, KK, 0 if j == 0 else 2, 0)
        gt += [(j, it, jt) for it in range((M + 63) // 64) for jt in range((N + 63) // 64)]
    gtab = ops._DeviceTable(gj, gt)
    cases.append(("gim_bgemm_grouped, 4 jobs of 80 x 512 x 512", lambda: lib.gim_bgemm_grouped(gtab.ptrs[0], gtab.ptrs[1], len(gt), st)))

    torch.cuda.synchronize()
    print("library: %s; %d rounds after %d warm-up calls; microseconds" % (L.LIB_PATH, a.rounds, a.warmup))
    print("%-75s %9s %9s %9s" % ("entry", "median", "min", "max"))
    for name, call in cases:
        for _ in range(a.warmup):
            L.check(call(), name)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        print("%-75s %9.1f %9.1f %9.1f" % (name, statistics.median(times), min(times), max(times)), flush=True)


if __name__ == "__main__":
    main()
