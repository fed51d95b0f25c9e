"""Measurements of the ArcFace baseline's training path (baseline_training.py, csrc/irse_train.hip) on one GPU.

    python tools/arcface_train_profile.py rate [B=128] [iters=20]      train_arcface-style iterations / s (sampler + gather + step),
                                                                       ArcFace-50 on 64x64x3 images, three repetitions
    python tools/arcface_train_profile.py census [B=32]                ATen operators that launch kernels inside one train_step
    python tools/arcface_train_profile.py unit                         device kernels of one IR-SE unit, forward and backward
    rocprofv3 --kernel-trace --stats -d DIR -o irse -- python tools/arcface_train_profile.py kernels
                                                                       the new map kernels alone (no counters in the same run)
    python tools/arcface_train_profile.py summarise DIR/..._kernel_trace.csv
                                                                       median time per kernel of that trace, as bytes moved / time

`kernels` runs one stage-1 map of a 128-image batch ([128, 32, 32, 64], 33.5 MB) through every new pass, forward and backward;
each call works on another of ROT buffers (ROT x 33.5 MB > the 256 MiB Infinity Cache), so no pass finds its map in a cache.  In a
training step the map was written by the kernel just before."""
import collections
import csv
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import optimalstrategiesagainstgenerativeattacks_amd as G  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd import ops  # noqa: E402
from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import irse_unit_train  # noqa: E402

SHAPE, ROT, REPS = (128, 32, 32, 64), 10, 8
PEAK_COPY = 6.29e12      # float4 copy, bytes / s
# bytes each kernel has to move, in units of the map's bytes Z (reads + writes; the subsample's small side is Z / 4)
MOVED = {"bn_stats_slab_kernel": 1.0, "bn_apply_fwd_kernel<false>": 2.0, "bn_apply_fwd_kernel<true>": 2.0, "bn_bwd_slab_kernel<false>": 2.0,
         "bn_bwd_slab_kernel<true>": 2.0, "bn_bwd_dx_kernel<false>": 3.0, "bn_bwd_dx_kernel<true>": 3.0, "prelu_fwd_kernel<true>": 2.0,
         "prelu_bwd_slab_kernel<true>": 3.0, "se_tail_kernel<false>": 3.0, "se_tail_bwd_kernel": 3.0, "subsample2_fwd_kernel": 0.5,
         "subsample2_bwd_kernel": 1.25, "dropout_kernel": 2.0}


def _trainer(B, dev, size=64, channels=3):
    imgs, offs = G.synthetic_bank(64, 20, size, channels, dev, seed=1)
    bank = G.EpisodeBank(imgs, offs, 1, 1, 1, mirror=True, seed=2)
    torch.manual_seed(0)
    model = G.ArcFace(G.Backbone(50, 0.6, 'ir_se', size, channels), 512, 64)
    with torch.no_grad():
        model.head.kernel.uniform_(-1, 1)
    return G.ArcFaceTrainer(model.to(dev)), G.IdentitySampler(bank, B, seed=3)


def rate(B, iters):
    dev = torch.device("cuda:0")
    tr, sampler = _trainer(B, dev)
    for it in range(3):
        x, label = sampler.batch(it)
        tr.train_step(x, label, it)
    torch.cuda.synchronize()
    rates = []
    for rep in range(3):
        t0 = time.perf_counter()
        for it in range(iters):
            x, label = sampler.batch(it)
            loss, acc = tr.train_step(x, label, it)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates.append(iters / dt)
        print("B = %d: %d iterations in %.3f s = %.2f iterations/s (%.0f images/s), last loss %.4f" % (B, iters, dt, iters / dt, B * iters / dt, float(loss)))
    print("spread over the repetitions: %.2f .. %.2f iterations/s" % (min(rates), max(rates)))
    print("peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def _profiled(fn, warm, steps):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    launched, stacks, kernels = collections.Counter(), collections.defaultdict(collections.Counter), collections.Counter()
    for ev in prof.events():
        if ev.name.startswith("aten::") and any(k.name for k in ev.kernels):
            launched[ev.name] += 1
            fr = [s for s in (ev.stack or []) if "optimalstrategies" in s]
            stacks[ev.name][" <- ".join(f.split("/")[-1] for f in fr[:2]) or "(autograd engine)"] += 1
        for k in ev.kernels:
            kernels[k.name.split("(")[0][:70]] += 1
    return launched, stacks, kernels


def census(B):
    dev = torch.device("cuda:0")
    tr, sampler = _trainer(B, dev)
    batches = [sampler.batch(it) for it in range(2)]
    state = [0]

    def step():
        x, label = batches[state[0] % 2]
        tr.train_step(x, label, state[0])
        state[0] += 1
    steps = 2
    launched, stacks, kernels = _profiled(step, 2, steps)
    print("ATen operators that launched kernels inside train_step, per step (B = %d, %d profiled steps):" % (B, steps))
    for name, c in launched.most_common():
        print("  %-20s %6.1f   %s" % (name, c / steps, dict((k, v / steps) for k, v in stacks[name].most_common(4))))
    if not launched:
        print("  none")
    print("device kernels per step (%.0f in all):" % (sum(kernels.values()) / steps))
    for name, c in kernels.most_common():
        print("  %6.1f  %s" % (c / steps, name))


def unit():
    """Launches of one (64, 64, 2), one (64, 128, 2) and one (128, 128, 1) unit, forward + backward, at N = 32."""
    dev = torch.device("cuda:0")
    from optimalstrategiesagainstgenerativeattacks_amd.baselines import _Unit
    for cin, depth, stride, S in ((64, 64, 2, 32), (64, 128, 2, 32), (128, 128, 1, 16)):
        u = _Unit(cin, depth, stride).to(dev)
        x = torch.randn(32, S, S, cin, device=dev).requires_grad_()

        def run():
            out = irse_unit_train(u, x)
            with ops.caller_thread_backward():
                out.backward(torch.ones_like(out))
            x.grad = None
        launched, _, kernels = _profiled(run, 2, 1)
        print("unit (%d, %d, %d) on %dx%d, N = 32: %d device kernels forward + backward" % (cin, depth, stride, S, S, sum(kernels.values())))
        for name, c in sorted(kernels.items()):
            print("  %3d  %s" % (c, name))
        print("  ATen operators among them: %s" % (dict(launched) or "none"))


def kernels():
    dev = torch.device("cuda:0")
    N, H, W, C = SHAPE
    xs = [torch.randn(SHAPE, device=dev).requires_grad_() for _ in range(ROT)]
    dys = [torch.randn(SHAPE, device=dev) for _ in range(ROT)]
    halves = [torch.randn(N, H // 2, W // 2, C, device=dev) for _ in range(ROT)]
    w, b = (1 + 0.3 * torch.randn(C, device=dev)).requires_grad_(), (0.3 * torch.randn(C, device=dev)).requires_grad_()
    a = (0.25 + 0.1 * torch.randn(C, device=dev)).requires_grad_()
    gate = torch.randn(N, C, device=dev).requires_grad_()
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    for rep in range(REPS + 2):
        for i, (x, dy, hf) in enumerate(zip(xs, dys, halves)):
            sc = xs[(i + 3) % ROT]
            for slope in (None, a):
                y = ops.batch_norm(x, w, b, rm, rv, nbt, 0.1, 1e-5, slope)
                torch.autograd.grad(y, (x, w, b), dy)
            torch.autograd.grad(ops.prelu(x, a), (x, a), dy)
            torch.autograd.grad(ops.se_tail_train(x, gate, sc, 1), (x, gate), dy)
            torch.autograd.grad(ops.subsample2(x), x, hf)
            torch.autograd.grad(ops.dropout(x, 0.6, 1, rep), x, dy)
    torch.cuda.synchronize()


def summarise(path):
    """Median over the dispatches of each kernel, the first two repetitions (code load, first touch of the buffers) dropped."""
    rows = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            rows[name].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    Z = 4.0
    for d in SHAPE:
        Z *= d
    print("map %s = %.1f MB, %d rotating buffers" % ("x".join(map(str, SHAPE)), Z / 1e6, ROT))
    print("%-32s %9s %10s %9s %7s %s" % ("kernel", "MB moved", "median us", "min us", "TB/s", "of the 6.29 TB/s copy rate"))
    for name in sorted(rows):
        ds = sorted(rows[name])
        ts = sorted(d for _, d in ds[len(ds) * 2 // (REPS + 2):])
        med = ts[len(ts) // 2]
        if name in MOVED:
            nbytes = MOVED[name] * Z
            print("%-32s %9.1f %10.2f %9.2f %7.2f %5.0f %%  (%d launches)" % (name, nbytes / 1e6, med, ts[0], nbytes / med / 1e6,
                                                                             100 * nbytes / (med * 1e-6) / PEAK_COPY, len(ts)))
        elif name.startswith(("ir_", "bn_")):
            print("%-32s %9s %10.2f %9.2f %7s        (%d launches)" % (name, "-", med, ts[0], "-", len(ts)))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rate"
    if mode == "rate":
        rate(int(sys.argv[2]) if len(sys.argv) > 2 else 128, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    elif mode == "census":
        census(int(sys.argv[2]) if len(sys.argv) > 2 else 32)
    elif mode == "unit":
        unit()
    elif mode == "kernels":
        kernels()
    elif mode == "summarise":
        summarise(sys.argv[2])
    else:
        raise SystemExit(__doc__)
