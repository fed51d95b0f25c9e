"""Measurements of the siamese baseline's training path (baseline_training.py, csrc/bn_train.hip) on one GPU.

    python tools/siamese_train_profile.py rate [B=128] [iters=300]     train_siamese-style iterations / s (sampler + gather + step)
    python tools/siamese_train_profile.py census [B=128]               ATen operators that launch kernels inside one train_step
    rocprofv3 --kernel-trace --stats -d DIR -o bn -- python tools/siamese_train_profile.py kernels
                                                                       the BatchNorm kernels alone at the training shapes
    python tools/siamese_train_profile.py summarise DIR/..._kernel_trace.csv
                                                                       median time per (kernel, shape) of that trace, as bytes moved / time

`kernels` runs the four blocks' maps of a 128-pair batch (256 images of 32x32 ... 4x4 pixels, 64 channels) through
ops.bn_relu_maxpool2 forward and backward; each call works on another of ROT buffers (ROT x 67 MB > the 256 MiB Infinity Cache at
the largest shape), so no pass finds its map in a cache.  In a training step the map was written by the convolution just before."""
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

IMAGES, C, SIZES, ROT, REPS = 256, 64, (32, 16, 8, 4), 6, 12
PEAK_COPY = 6.29e12      # float4 copy, bytes / s


def _trainer(B, dev):
    imgs, offs = G.synthetic_bank(64, 20, 32, 1, dev, seed=1)
    bank = G.EpisodeBank(imgs, offs, 1, 1, 1, mirror=True, seed=2)
    torch.manual_seed(0)
    net = G.ProtonetEmbeddingNet(1, 32)
    tr = G.SiameseTrainer(G.SiameseNet(net, net.embedding_dim).to(dev))
    return tr, G.PairSampler(bank, B, seed=3)


def rate(B, iters):
    dev = torch.device("cuda:0")
    tr, sampler = _trainer(B, dev)
    for it in range(20):
        tr.train_step(*sampler.batch(it))
    torch.cuda.synchronize()
    for rep in range(3):
        t0 = time.perf_counter()
        for it in range(iters):
            loss, acc = tr.train_step(*sampler.batch(it))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print("B = %d: %d iterations in %.3f s = %.1f iterations/s (%.0f pairs/s), last loss %.4f" % (B, iters, dt, iters / dt, B * iters / dt, float(loss)))


def census(B):
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    tr, sampler = _trainer(B, dev)
    batches = [sampler.batch(it) for it in range(5)]
    for b in batches[:3]:
        tr.train_step(*b)
    torch.cuda.synchronize()
    steps = 2
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
        for b in batches[3:]:
            tr.train_step(*b)
        torch.cuda.synchronize()
    launched, stacks, kernels = collections.Counter(), collections.defaultdict(collections.Counter), collections.Counter()
    for ev in prof.events():
        if ev.name.startswith("aten::") and any(k.name for k in ev.kernels):
            launched[ev.name] += 1
            fr = [s for s in (ev.stack or []) if "optimalstrategies" in s]
            stacks[ev.name][" <- ".join(f.split("/")[-1] for f in fr[:2]) or "(autograd engine)"] += 1
        for k in ev.kernels:
            kernels[k.name.split("(")[0][:70]] += 1
    print("ATen operators that launched kernels inside train_step, per step (B = %d, %d profiled steps):" % (B, steps))
    for name, c in launched.most_common():
        print("  %-20s %5.1f   %s" % (name, c / steps, dict((k, v / steps) for k, v in stacks[name].most_common(4))))
    if not launched:
        print("  none")
    print("device kernels per step:")
    for name, c in kernels.most_common():
        print("  %5.1f  %s" % (c / steps, name))


def kernels():
    dev = torch.device("cuda:0")
    for S in SIZES:
        zs = [torch.randn(IMAGES, S, S, C, device=dev).requires_grad_() for _ in range(ROT if S == SIZES[0] else 2 * ROT)]
        w, b = (1 + 0.3 * torch.randn(C, device=dev)).requires_grad_(), (0.3 * torch.randn(C, device=dev)).requires_grad_()
        rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        dps = [torch.randn(IMAGES, S // 2, S // 2, C, device=dev) for _ in zs]
        for rep in range(REPS + 2):
            for z, dp in zip(zs, dps):
                p = ops.bn_relu_maxpool2(z, w, b, rm, rv, nbt)
                torch.autograd.grad(p, (z, w, b), dp)
        torch.cuda.synchronize()
        del zs, dps


def summarise(path):
    """Per kernel and map size: the dispatches of a kernel in time order are those of `kernels` - len(zs) * (REPS + 2) per size,
    sizes in the order of SIZES; the first two repetitions of every size (code load, first touch of the buffers) are dropped."""
    rows = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if name.startswith(("bn_", "rowsum_")):
                wg = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) // (int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]))
                rows[name].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, wg))
    # bytes each kernel has to move at a map of Z bytes: stats reads z; forward reads z, writes z / 4; the backward sums read z and
    # dp (z / 4); dz reads z and dp and writes z; the two stage-2 kernels (bn_finalize_kernel, rowsum_finalize_kernel) read 8 bytes per channel and
    # slab
    moved = {"bn_stats_slab_kernel": 1.0, "bn_relu_maxpool2_fwd_kernel": 1.25, "bn_pool_bwd_slab_kernel": 1.25, "bn_pool_bwd_dx_kernel": 2.25}
    print("%-32s %8s %10s %9s %9s %8s %s" % ("kernel", "map", "MB moved", "median us", "min us", "TB/s", "of the 6.29 TB/s copy rate"))
    for name in sorted(rows):
        ds = sorted(rows[name])
        pos = 0
        for S in SIZES:
            n_buf = ROT if S == SIZES[0] else 2 * ROT
            seg = ds[pos:pos + n_buf * (REPS + 2)]
            pos += n_buf * (REPS + 2)
            ts = sorted(d for _, d, _ in seg[2 * n_buf:])
            if not ts:
                continue
            med, wg = ts[len(ts) // 2], seg[-1][2]
            if name in moved:
                nbytes = moved[name] * IMAGES * S * S * C * 4
                print("%-32s %3dx%-3d %9.2f %10.2f %9.2f %8.2f %5.0f %%  (%d launches, %d workgroups)"
                      % (name, S, S, nbytes / 1e6, med, ts[0], nbytes / med / 1e6, 100 * nbytes / (med * 1e-6) / PEAK_COPY, len(ts), wg))
            else:
                print("%-32s %3dx%-3d %9s %10.2f %9.2f %8s        (%d launches, %d workgroups)" % (name, S, S, "-", med, ts[0], "-", len(ts), wg))
        assert pos == len(ds), (name, pos, len(ds))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rate"
    if mode == "rate":
        rate(int(sys.argv[2]) if len(sys.argv) > 2 else 128, int(sys.argv[3]) if len(sys.argv) > 3 else 300)
    elif mode == "census":
        census(int(sys.argv[2]) if len(sys.argv) > 2 else 128)
    elif mode == "kernels":
        kernels()
    elif mode == "summarise":
        summarise(sys.argv[2])
    else:
        raise SystemExit(__doc__)
