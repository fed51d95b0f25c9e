"""BatchNorm over the ranks of a data-parallel step (ops.bn_stats_record / bn_stats_merge, the total_rows argument of the two dz
passes, the sync argument of ops.batch_norm / ops.bn_relu_maxpool2) in ONE process: the shards of a batch run one after the other
through the primitives, their sums are added in rank order as the all-reduce adds them, and the concatenated results are compared
with fp64 torch on the WHOLE batch (F.batch_norm(training=True), autograd for the gradients).  Every bound is the one the project
already holds the same quantity to (tests/test_gpu_bn_train.py, tests/test_gpu_irse_train.py).  Every test is a single shot."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests import test_gpu_bn_train as bt
from tests.helpers import T, relerr

TOL = 3e-5          # relative L2, fp32 kernels against fp64
TOL_DZ = 2e-4       # dz of the pooled family
TOL_MAX = 2e-4      # largest single-element error of p relative to the largest reference element
MOMENTUM, EPS = 0.1, 1e-5

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ops_mod():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    return ops


def f32(t):
    return t.float().to(dev()).contiguous()


def cut(t, shards):
    assert sum(shards) == t.shape[0]
    return list(torch.split(t, list(shards), 0))


def rows_of(t):
    return t.numel() // t.shape[-1]


def running(tag, C):
    return T(0.2 * pf.uniform(tag + "/rm", (C,))).float(), T(1.0 + 0.5 * np.abs(pf.uniform(tag + "/rv", (C,)))).float()


def merged_stats(ops, shards, rm=None, rv=None, nbt=None):
    """(mean, invstd) from the shards' records, merged in rank order; the running statistics move where given."""
    records = torch.stack([ops.bn_stats_record(f32(s)) for s in shards])
    assert records.shape == (len(shards), 2, shards[0].shape[-1])
    return ops.bn_stats_merge(records, [rows_of(s) for s in shards], EPS, rm, rv, nbt, MOMENTUM)


def stats_reference(z, rm0, rv0):
    """fp64 torch on the whole batch z [..., C] (the fp32 values, widened)."""
    x = z.double().reshape(-1, z.shape[-1])
    rm, rv = rm0.double().clone(), rv0.double().clone()
    F.batch_norm(x, rm, rv, None, None, training=True, momentum=MOMENTUM, eps=EPS)
    return dict(mean=x.mean(0), invstd=1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS), rm=rm, rv=rv)


def check_stats(tag, z, shards):
    ops = ops_mod()
    C = z.shape[-1]
    rm0, rv0 = running(tag, C)
    ref = stats_reference(z, rm0, rv0)
    rm, rv, nbt = f32(rm0), f32(rv0), torch.tensor(7, dtype=torch.int64, device=dev())
    mean, invstd = merged_stats(ops, cut(z, shards), rm, rv, nbt)
    errs = {k: relerr(v, ref[k]) for k, v in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv))}
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < TOL, (tag, k, e)
    assert int(nbt) == 8
    return ref


# ---------------------------------------------------------------------------------------------------- statistics
ROW_SHARDS = {
    "1+3x8": ((1, 3), 8),                # BatchNorm1d with a one-row rank; the unbiased factor 4 / 3
    "5+1+130x132": ((5, 1, 130), 132),   # three ranks, unequal counts, one shard of three slabs, a channel count off the 64-channel block
    "4100+61x8": ((4100, 61), 8),        # 65 slabs on one rank: a thread of the combine has two
}


@pytest.mark.parametrize("name", list(ROW_SHARDS))
def test_merged_statistics_of_row_shards(name):
    shards, C = ROW_SHARDS[name]
    ops = ops_mod()
    if name == "5+1+130x132":
        assert ops.bn_slabs(130) == 3
    if name == "4100+61x8":
        assert ops.bn_slabs(4100) == 65
    tag = "bnsync/rows/" + name
    z = T(0.5 + 1.5 * pf.normal(tag + "/z", (sum(shards), C))).float()
    ref = check_stats(tag, z, shards)
    if name == "1+3x8":       # the running variance moved with M2 / 3, not M2 / 4
        x = z.double()
        assert relerr(ref["rv"], 0.9 * running(tag, C)[1].double() + 0.1 * x.var(0, unbiased=False) * 4.0 / 3.0) < 1e-12


def test_merged_statistics_of_a_map_cut_along_n():
    tag = "bnsync/map"
    z = T(0.5 + 1.5 * pf.normal(tag + "/z", (4, 32, 32, 64))).float()
    check_stats(tag, z, (1, 3))


def test_sixty_four_ranks_of_one_row_each():
    """The stated maximum R; every record is (the row, 0)."""
    ops = ops_mod()
    tag = "bnsync/r64"
    z = T(pf.normal(tag + "/z", (64, 8))).float()
    rec = ops.bn_stats_record(f32(z[5:6]))
    assert torch.equal(rec[0].cpu(), z[5]) and float(rec[1].abs().max()) == 0.0
    check_stats(tag, z, (1,) * 64)


def test_shard_means_far_apart_on_a_common_offset():
    """Rank 0 is N(0, 1), rank 1 is N(50, 1), both on a level of 1000: the variance of the whole is ~626, the shards' own ~1.
    Averaging the shard variances, or E[x^2] - E[x]^2 in fp32 at this level, fails the bound."""
    tag = "bnsync/far"
    a, b = pf.normal(tag + "/a", (192, 8)), 50.0 + pf.normal(tag + "/b", (192, 8))
    z = T(np.concatenate([a, b]) + 1000.0).float()
    ref = check_stats(tag, z, (192, 192))
    x = z.double()
    naive = 1.0 / torch.sqrt(0.5 * (x[:192].var(0, unbiased=False) + x[192:].var(0, unbiased=False)) + EPS)
    assert relerr(naive, ref["invstd"]) > 1.0 and float(ref["mean"].min()) > 1000.0


@pytest.mark.parametrize("rows", [48, 4100], ids=["one_slab", "65_slabs"])
def test_one_rank_is_bn_stats_bit_for_bit(rows):
    ops = ops_mod()
    assert ops.bn_slabs(rows) == (1 if rows == 48 else 65)
    tag = "bnsync/r1/%d" % rows
    z = f32(T(0.5 + 1.5 * pf.normal(tag + "/z", (rows, 8))))
    rm0, rv0 = running(tag, 8)
    rm_a, rv_a, rm_b, rv_b = f32(rm0), f32(rv0), f32(rm0), f32(rv0)
    nbt_a, nbt_b = (torch.tensor(7, dtype=torch.int64, device=dev()) for _ in range(2))
    mean_a, invstd_a = ops.bn_stats(z, EPS, rm_a, rv_a, nbt_a, MOMENTUM)
    mean_b, invstd_b = ops.bn_stats_merge(ops.bn_stats_record(z)[None], [rows], EPS, rm_b, rv_b, nbt_b, MOMENTUM)
    for k, u, v in (("mean", mean_a, mean_b), ("invstd", invstd_a, invstd_b), ("rm", rm_a, rm_b), ("rv", rv_a, rv_b)):
        assert torch.equal(u, v), (k, float((u - v).abs().max()))
    assert int(nbt_a) == int(nbt_b) == 8
    assert not torch.equal(rm_a, f32(rm0))


def test_refusals():
    ops = ops_mod()
    rec = torch.zeros(3, 2, 8, device=dev())
    with pytest.raises(RuntimeError, match="at least two rows"):
        ops.bn_stats_merge(rec[:1], [1], EPS)
    with pytest.raises(RuntimeError, match="at least 1"):
        ops.bn_stats_merge(rec, [4, 0, 4], EPS)
    with pytest.raises(RuntimeError, match="R <= 64"):
        ops.bn_stats_merge(torch.zeros(65, 2, 8, device=dev()), [2] * 65, EPS)
    with pytest.raises(RuntimeError, match="row counts"):
        ops.bn_stats_merge(rec, [4, 4], EPS)
    with pytest.raises(RuntimeError, match="C % 4"):
        ops.bn_stats_merge(torch.zeros(2, 2, 6, device=dev()), [2, 2], EPS)
    with pytest.raises(RuntimeError, match="C % 4"):
        ops.bn_stats_record(torch.zeros(3, 6, device=dev()))
    v = torch.ones(8, device=dev())
    with pytest.raises(RuntimeError, match="M_total"):
        ops.bn_bwd_dx(torch.zeros(4, 8, device=dev()), torch.zeros(4, 8, device=dev()), v, v, v, v, None, torch.zeros(2, 8, device=dev()), total_rows=3)


# ---------------------------------------------------------------------------------------------------- backward: batch_norm
_BN_REF = {}


def bn_reference(tag, z, gamma, beta, slope, dy, dtype=torch.float64):
    """torch on the whole batch; computed once per (tag, dtype)."""
    key = (tag, dtype)
    if key in _BN_REF:
        return _BN_REF[key]
    C = z.shape[-1]
    x = z.to(dtype).reshape(-1, C).clone().requires_grad_()
    gm, bb = gamma.to(dtype).clone().requires_grad_(), beta.to(dtype).clone().requires_grad_()
    yh = F.batch_norm(x, None, None, gm, bb, training=True, momentum=MOMENTUM, eps=EPS)
    ref = {}
    if slope is not None:
        if dtype == torch.float64:
            margin = float(yh.detach().abs().min())
            print("    %s: smallest |yhat| in front of the PReLU %.3e" % (tag, margin))
            assert margin > 2e-6, margin
        a = slope.to(dtype).clone().requires_grad_()
        y = F.prelu(yh, a)
    else:
        y = yh
    (y * dy.to(dtype).reshape(-1, C)).sum().backward()
    ref.update(y=y.detach().reshape(z.shape), dz=x.grad.reshape(z.shape), dgamma=gm.grad, dbeta=bb.grad)
    if slope is not None:
        ref["dslope"] = a.grad
    _BN_REF[key] = ref
    return ref


def bn_inputs(tag, shape, prelu):
    C = shape[-1]
    z = T(0.5 + 1.5 * pf.normal(tag + "/z", shape)).float()
    gamma = T(1.0 + 0.3 * pf.uniform(tag + "/gamma", (C,))).float()
    gamma[1::4] *= -1.0
    beta = T(0.3 * pf.uniform(tag + "/beta", (C,))).float()
    slope = None
    if prelu:
        slope = T(0.25 * (1.0 + 0.5 * pf.uniform(tag + "/a", (C,)))).float()
        slope[1::2] *= -1.0
    return z, gamma, beta, slope, T(pf.uniform(tag + "/dy", shape)).float()


def bn_sharded(ops, shards_z, shards_dy, gamma, beta, slope):
    """The data-parallel step of the shards, one after the other: merged statistics, local sums, their sum in rank order, dz."""
    gm, bb, sl = f32(gamma), f32(beta), None if slope is None else f32(slope)
    zs, dys = [f32(s) for s in shards_z], [f32(s) for s in shards_dy]
    mean, invstd = merged_stats(ops, zs)
    y = [ops.bn_apply(z, gm, bb, mean, invstd, sl) for z in zs]
    sums = [ops.bn_bwd_sums(dy, z, gm, bb, mean, invstd, sl) for dy, z in zip(dys, zs)]
    total = sums[0].clone()
    for s in sums[1:]:
        total += s
    M_total = sum(rows_of(z) for z in zs)
    dz = [ops.bn_bwd_dx(dy, z, gm, bb, mean, invstd, sl, total, total_rows=M_total) for dy, z in zip(dys, zs)]
    out = dict(y=torch.cat(y), dz=torch.cat(dz), dgamma=total[0], dbeta=total[1])
    if sl is not None:
        out["dslope"] = total[2]
    return out, sums, (mean, invstd)


BN_CASES = {
    "1+3x8": ((4, 8), (1, 3)),
    "5+1+130x132": ((136, 132), (5, 1, 130)),
    "map_1+3": ((4, 8, 8, 64), (1, 3)),
}


@pytest.mark.parametrize("prelu", [False, True], ids=["plain", "prelu"])
@pytest.mark.parametrize("name", list(BN_CASES))
def test_batch_norm_backward_over_shards(name, prelu):
    ops = ops_mod()
    shape, shards = BN_CASES[name]
    tag = "bnsync/bn/%s/%d" % (name, prelu)
    z, gamma, beta, slope, dy = bn_inputs(tag, shape, prelu)
    ref = bn_reference(tag, z, gamma, beta, slope, dy)
    bounds = {}
    if name == "1+3x8":
        # four rows: dz cancels heavily (the rule of test_batch_norm at M = 2): max(3 x torch's own fp32-vs-fp64 deviation, TOL)
        floor = relerr(bn_reference(tag, z, gamma, beta, slope, dy, torch.float32)["dz"], ref["dz"])
        bounds["dz"] = max(3.0 * floor, TOL)
        print("    torch's own fp32 dz at M = 4: %.3e -> bound %.3e" % (floor, bounds["dz"]))
    got, _, _ = bn_sharded(ops, cut(z, shards), cut(dy, shards), gamma, beta, slope)
    errs = {k: relerr(got[k], ref[k]) for k in ref}
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in errs.items())))
    for k, e in errs.items():
        assert e < bounds.get(k, TOL), (tag, k, e)


# ---------------------------------------------------------------------------------------------------- backward: bn_relu_maxpool2
POOL_CASES = {
    "4x4x8x64": ((4, 4, 8, 64), (1, 3)),
    "2x2x2x132": ((2, 2, 2, 132), (1, 1)),
}
POOL_FILL = {}      # fill names whose fp64 reference has the margins of tests/test_gpu_bn_train.py (asserted by its reference())


def pool_case(name):
    (N, H, W, C), shards = POOL_CASES[name]
    tag = "bnsync/pool/" + name + POOL_FILL.get(name, "")
    z, (gamma, beta) = bt.grid_map(tag, N, H, W, C), bt.affine(tag, C)
    dp = T(pf.uniform(tag + "/dp", (N, H // 2, W // 2, C)))
    return tag, shards, z, gamma, beta, dp, bt.reference(tag, z, gamma, beta, dp)      # asserts gap and |max| > MARGIN in fp64


def pool_sharded(ops, shards_z, shards_dp, gamma, beta, rm=None, rv=None, nbt=None):
    gm, bb = f32(gamma), f32(beta)
    zs, dps = [f32(s) for s in shards_z], [f32(s) for s in shards_dp]
    mean, invstd = merged_stats(ops, zs, rm, rv, nbt)
    p = [ops.bn_pool_fwd(z, gm, bb, mean, invstd) for z in zs]
    sums = [ops.bn_pool_bwd_sums(dp, z, gm, bb, mean, invstd) for dp, z in zip(dps, zs)]
    total = sums[0].clone()
    for s in sums[1:]:
        total += s
    M_total = sum(rows_of(z) for z in zs)
    dz = [ops.bn_pool_bwd_dx(dp, z, gm, bb, mean, invstd, total, total_rows=M_total) for dp, z in zip(dps, zs)]
    return dict(p=torch.cat(p), dz=torch.cat(dz), dgamma=total[0], dbeta=total[1], mean=mean, invstd=invstd), sums, (mean, invstd)


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_bn_relu_maxpool2_backward_over_shards(name):
    ops = ops_mod()
    tag, shards, z, gamma, beta, dp, ref = pool_case(name)
    rm, rv, nbt = f32(ref["rm0"]), f32(ref["rv0"]), torch.tensor(7, dtype=torch.int64, device=dev())
    got, _, _ = pool_sharded(ops, cut(z, shards), cut(dp, shards), gamma, beta, rm, rv, nbt)
    got.update(rm=rm, rv=rv)
    errs = {k: relerr(got[k], ref[k]) for k in ("p", "dz", "dgamma", "dbeta", "mean", "invstd", "rm", "rv")}
    emax = float((got["p"].double().cpu() - ref["p"]).abs().max() / ref["p"].abs().max())
    print("%s: %s, p max element %.2e" % (tag, " ".join("%s %.2e" % kv for kv in errs.items()), emax))
    for k, e in errs.items():
        assert e < (TOL_DZ if k == "dz" else TOL), (tag, k, e)
    assert emax < TOL_MAX, (tag, emax)
    assert int(nbt) == 8


# ---------------------------------------------------------------------------------------------------- the sync argument, one process
class PeerSync:
    """Rank 0 of two, the peer's contributions computed beforehand: all_gather stacks the peer's record behind this rank's,
    all_reduce_ adds the peer's sums.  Records what passed through."""
    rank, world = 0, 2

    def __init__(self, peer_record, peer_sums):
        self.peer_record, self.peer_sums = peer_record, peer_sums
        self.gathered, self.reduced = [], []

    def all_gather(self, t):
        self.gathered.append(t.clone())
        return torch.stack([t, self.peer_record])

    def all_reduce_(self, t):
        self.reduced.append(t.clone())
        t += self.peer_sums[:t.shape[0]]
        return t


def bucket_views(*params):
    """.grad of every parameter as a view of ONE flat buffer holding 0.25, as FusedAdam's bucket."""
    flat = torch.full((sum(p.numel() for p in params),), 0.25, device=dev())
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat


@pytest.mark.parametrize("prelu", [False, True], ids=["plain", "prelu"])
def test_batch_norm_sync_keeps_the_local_sums_in_the_bucket(prelu):
    """ops.batch_norm(sync=...) on rank 0's half: y and dz are the whole batch's (bit-equal to the primitives' path), the running
    statistics are the whole batch's - and what is ADDED to the optimizer's bucket is the LOCAL sum: FusedAdam.step all-reduces the
    bucket once more, the totals there would count every rank `world` times."""
    ops = ops_mod()
    tag = "bnsync/bucket/%d" % prelu
    z, gamma, beta, slope, dy = bn_inputs(tag, (8, 16), prelu)
    ref = bn_reference(tag, z, gamma, beta, slope, dy)
    zs, dys = cut(z, (4, 4)), cut(dy, (4, 4))
    want, sums, _ = bn_sharded(ops, zs, dys, gamma, beta, slope)
    sync = PeerSync(ops.bn_stats_record(f32(zs[1])), sums[1])
    zg = f32(zs[0]).requires_grad_()
    params = [f32(t).requires_grad_() for t in (gamma, beta, slope) if t is not None]
    flat = bucket_views(*params)
    rm0, rv0 = running(tag, 16)
    rm, rv, nbt = f32(rm0), f32(rv0), torch.tensor(7, dtype=torch.int64, device=dev())
    y = ops.batch_norm(zg, params[0], params[1], rm, rv, nbt, MOMENTUM, EPS, params[2] if prelu else None, sync=sync)
    y.backward(f32(dys[0]))
    assert torch.equal(y.detach(), want["y"][:4]) and torch.equal(zg.grad, want["dz"][:4])
    assert len(sync.gathered) == 1 and len(sync.reduced) == 1 and tuple(sync.reduced[0].shape) == (2, 16)      # dslope stays home
    assert torch.equal(sync.reduced[0], sums[0][:2])
    sref = stats_reference(z, rm0, rv0)
    assert relerr(rm, sref["rm"]) < TOL and relerr(rv, sref["rv"]) < TOL and int(nbt) == 8
    added = (flat - 0.25).view(len(params), 16)
    for i, k in enumerate(("dgamma", "dbeta", "dslope")[:len(params)]):
        local, total = sums[0][i], want[k]
        e_local, e_total = relerr(added[i], local), relerr(added[i], total)
        print("%s bucket %s: %.2e from the local sum, %.2e from the total (total against fp64: %.2e)" % (tag, k, e_local, e_total, relerr(total, ref[k])))
        assert e_local < TOL and e_total > 1e-2, (k, e_local, e_total)      # (0.25 + s) - 0.25: two roundings of the bucket's element
    # without a bucket the local sums go back to autograd
    zg2 = f32(zs[0]).requires_grad_()
    params2 = [f32(t).requires_grad_() for t in (gamma, beta, slope) if t is not None]
    y2 = ops.batch_norm(zg2, params2[0], params2[1], None, None, None, MOMENTUM, EPS, params2[2] if prelu else None, sync=sync)
    grads = torch.autograd.grad(y2, [zg2] + params2, f32(dys[0]))
    assert torch.equal(grads[0], want["dz"][:4])
    for i in range(len(params2)):
        assert torch.equal(grads[1 + i], sums[0][i])


def test_bn_relu_maxpool2_sync_keeps_the_local_sums_in_the_bucket():
    ops = ops_mod()
    tag, shards, z, gamma, beta, dp, ref = pool_case("2x2x2x132")
    zs, dps = cut(z, shards), cut(dp, shards)
    want, sums, _ = pool_sharded(ops, zs, dps, gamma, beta)
    sync = PeerSync(ops.bn_stats_record(f32(zs[1])), sums[1])
    zg, gg, bg = f32(zs[0]).requires_grad_(), f32(gamma).requires_grad_(), f32(beta).requires_grad_()
    flat = bucket_views(gg, bg)
    rm, rv, nbt = f32(ref["rm0"]), f32(ref["rv0"]), torch.tensor(7, dtype=torch.int64, device=dev())
    p = ops.bn_relu_maxpool2(zg, gg, bg, rm, rv, nbt, MOMENTUM, EPS, sync=sync)
    p.backward(f32(dps[0]))
    assert torch.equal(p.detach(), want["p"][:1]) and torch.equal(zg.grad, want["dz"][:1])
    assert relerr(rm, ref["rm"]) < TOL and relerr(rv, ref["rv"]) < TOL and int(nbt) == 8
    added = (flat - 0.25).view(2, 132)
    for i, k in enumerate(("dgamma", "dbeta")):
        e_local, e_total = relerr(added[i], sums[0][i]), relerr(added[i], want[k])
        print("%s bucket %s: %.2e from the local sum, %.2e from the total" % (tag, k, e_local, e_total))
        assert e_local < TOL and e_total > 1e-2, (k, e_local, e_total)


def test_world_of_one_takes_the_single_process_path():
    ops = ops_mod()

    class Alone:
        rank, world = 0, 1

        def all_gather(self, t):
            raise AssertionError("no collective at world == 1")
        all_reduce_ = all_gather
    tag = "bnsync/alone"
    z, gamma, beta, slope, dy = bn_inputs(tag, (6, 8), True)
    out = []
    for sync in (None, Alone()):
        zg, gm, bb, sl = (f32(t).requires_grad_() for t in (z, gamma, beta, slope))
        y = ops.batch_norm(zg, gm, bb, None, None, None, MOMENTUM, EPS, sl, sync=sync)
        out.append([y.detach()] + list(torch.autograd.grad(y, (zg, gm, bb, sl), f32(dy))))
    for u, v in zip(*out):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("it", [0, 3])
def test_dropout_mask_of_a_rank_is_its_rows_mask_in_the_whole_batch(it):
    ops = ops_mod()
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import dropout_offset
    x = f32(T(pf.normal("bnsync/drop/x", (8, 2, 2, 512))))
    whole = ops.dropout(x, 0.6, 11, dropout_offset(it, x.numel()))
    halves = [ops.dropout(x[4 * r:4 * r + 4].contiguous(), 0.6, 11, dropout_offset(it, x.numel() // 2, r, 2)) for r in (0, 1)]
    assert torch.equal(torch.cat(halves), whole)
    kept = float((whole != 0).float().mean())
    assert 0.35 < kept < 0.45 and not torch.equal(halves[0] != 0, halves[1] != 0)
    if it:
        assert not torch.equal(whole, ops.dropout(x, 0.6, 11, dropout_offset(0, x.numel())))
