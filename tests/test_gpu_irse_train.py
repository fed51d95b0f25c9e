"""The training passes of the ArcFace baseline that are not convolutions (csrc/irse_train.hip through the autograd Functions of
ops.py) against fp64 torch on the CPU at the project's operator bound, 3e-5 relative L2; then whole IR-SE units in training mode
against what the REFERENCE's bottleneck_IR_SE gave (tests/golden/arcface_train.npz, part (a)) at the block bound, 1e-4.

Inputs are rounded to fp32 before either side sees them.  Where a pass takes a decision (the sign in front of a PReLU, the margin
branch, the clamp) the case first asserts on the fp64 side that no element sits close enough to the decision for a rounding to flip
it.  Every case runs twice and the two runs are torch.equal: no pass combines partial sums in an order that varies."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests import arcface_fill as af
from tests import baseline_fill as bf
from tests.helpers import load_npz, relerr

TOL = 3e-5          # relative L2, fp32 kernels against fp64
BLOCK = 1e-4        # a block of several operators against the reference
MOMENTUM, EPS = 0.1, 1e-5

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ops_mod():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    return ops


def rnd(tag, shape, scale=1.0):
    """fp32 CPU tensor; .double() of it is what the fp64 side computes on."""
    return torch.from_numpy(np.ascontiguousarray(pf.normal(tag, tuple(shape)) * scale)).float()


def uni(tag, shape):
    return torch.from_numpy(np.ascontiguousarray(pf.uniform(tag, tuple(shape)))).float()


def g(t):
    return t.to(dev()).requires_grad_()


def twice(fn):
    """fn() -> dict of tensors, run twice: bit-identical; returns the first."""
    a, b = fn(), fn()
    for k in a:
        assert torch.equal(a[k], b[k]), "two runs differ in " + k
    return a


def close(got, ref, names=None, tol=TOL):
    for k in (names or ref):
        e = relerr(got[k], ref[k])
        print("    %-12s %.3e" % (k, e))
        assert e < tol, (k, e)


# ---------------------------------------------------------------------------------------------------- BatchNorm
BN_SHAPES = [(3, 6, 6, 8), (2, 5, 7, 24), (8, 512), (2, 64), (4, 32, 32, 64), (4161, 8), (65537, 4)]
# more slabs than the 64 lanes of the sums' stage 2, so that a lane adds a second slab: 66 slabs of 64 rows (lanes 0 and 1 add two,
# the last slab holds one row), and 1009 slabs of 65 rows at the cap of 1024 (the last one holds 17)
BN_SLABS = {(4161, 8): 66, (65537, 4): 1009}


def bn_inputs(tag, shape, prelu):
    C = shape[-1]
    z = rnd(tag + "/z", shape, 1.5) + 0.5 * uni(tag + "/off", (C,))
    gamma = 1.0 + 0.3 * uni(tag + "/gamma", (C,))
    gamma[1::4] *= -1.0
    beta = 0.3 * uni(tag + "/beta", (C,))
    slope = 0.25 * (1.0 + 0.5 * uni(tag + "/slope", (C,))) if prelu else None
    if prelu:
        slope[2::4] *= -1.0
    rm, rv = 0.2 * uni(tag + "/rm", (C,)), 1.0 + 0.5 * uni(tag + "/rv", (C,)).abs()
    if prelu:       # move the few elements that the normalisation would put within 1e-3 of the PReLU's kink (bn_reference checks the result)
        yh = F.batch_norm(z.double().reshape(-1, C), None, None, gamma.double(), beta.double(), training=True, eps=EPS).reshape(shape)
        z = torch.where(yh.abs() < 1e-3, z + 0.02, z)
    return z, gamma, beta, slope, rm, rv, rnd(tag + "/dy", shape)


def bn_reference(z, gamma, beta, slope, rm, rv, dy, dtype=torch.float64):
    """torch on the CPU, in fp64 (the reference) or in fp32 (torch's own deviation from it)."""
    C = z.shape[-1]
    x = z.to(dtype).reshape(-1, C).clone().requires_grad_()      # (clones: .to() of an fp32 input is the input itself)
    gm, bt = gamma.to(dtype).clone().requires_grad_(), beta.to(dtype).clone().requires_grad_()
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    yh = F.batch_norm(x, rm, rv, gm, bt, training=True, momentum=MOMENTUM, eps=EPS)
    ref = {}
    if slope is not None:
        margin = float(yh.detach().abs().min())
        print("    smallest |yhat| in front of the PReLU %.3e" % margin)
        assert margin > 2e-6, margin
        a = slope.to(dtype).clone().requires_grad_()
        y = F.prelu(yh, a)
    else:
        y = yh
    (y * dy.to(dtype).reshape(-1, C)).sum().backward()
    ref.update(y=y.detach().reshape(z.shape), dz=x.grad.reshape(z.shape), dgamma=gm.grad, dbeta=bt.grad, rm=rm, rv=rv)
    if slope is not None:
        ref["dslope"] = a.grad
    return ref


def bn_run(z, gamma, beta, slope, rm, rv, dy, bucket):
    ops = ops_mod()
    zg, gm, bt = g(z), g(gamma), g(beta)
    sl = None if slope is None else g(slope)
    params = [p for p in (gm, bt, sl) if p is not None]
    if bucket:      # the gradients are added into existing .grad buffers, as into FusedAdam's bucket
        for p in params:
            p.grad = torch.full_like(p.detach(), 0.25)
    rmg, rvg = rm.to(dev()), rv.to(dev())
    nbt = torch.tensor(7, dtype=torch.int64, device=dev())
    y = ops.batch_norm(zg, gm, bt, rmg, rvg, nbt, MOMENTUM, EPS, sl)
    if bucket:
        y.backward(dy.to(dev()))
        grads = [zg.grad] + [p.grad - 0.25 for p in params]
    else:
        grads = list(torch.autograd.grad(y, [zg] + params, dy.to(dev())))
    assert int(nbt) == 8
    out = dict(y=y.detach(), dz=grads[0], dgamma=grads[1], dbeta=grads[2], rm=rmg, rv=rvg)
    if sl is not None:
        out["dslope"] = grads[3]
    return out


@pytest.mark.parametrize("prelu", [False, True], ids=["plain", "prelu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_norm(shape, prelu):
    tag = "irse/bn/%s/%d" % ("x".join(map(str, shape)), prelu)
    inp = bn_inputs(tag, shape, prelu)
    ref = bn_reference(*inp)
    M = inp[0].numel() // shape[-1]
    if shape in BN_SLABS:
        assert ops_mod().bn_slabs(M) == BN_SLABS[shape]
    bounds = {}
    if M == 2:
        # two rows: xhat = +-1 / sqrt(1 + eps / var), and dz = gamma * invstd * (dyhat - mean - xhat * mean(dyhat * xhat)) cancels to
        # O(eps / var) of its terms - in exact arithmetic and in either precision, so no fp32 implementation reaches 3e-5 against dz
        # itself.  The bound on dz is the project's usual one: max(3 x torch's own fp32-vs-fp64 deviation, 3e-5), measured here.
        floor = relerr(bn_reference(*inp, dtype=torch.float32)["dz"], ref["dz"])
        bounds["dz"] = max(3.0 * floor, TOL)
        print("    torch's own fp32 dz at M = 2: %.3e -> bound %.3e" % (floor, bounds["dz"]))
    for bucket in (False, True):
        got = twice(lambda: bn_run(*inp, bucket=bucket))
        for k in ref:
            e = relerr(got[k], ref[k])
            print("    %-12s %.3e" % (k, e))
            assert e < bounds.get(k, TOL), (k, e)


def test_batch_norm_offset_map_keeps_its_variance():
    """z + 1024 on a grid of eighths (exact in fp32): a spread of ~2.3 on a level of 1024, which E[x^2] - E[x]^2 would lose."""
    ops = ops_mod()
    z = torch.from_numpy(np.rint(pf.normal("irse/bn/offset", (2, 8, 8, 8)) * 16.0) / 8.0 + 1024.0).float()
    x = z.double().reshape(-1, 8)
    rm, rv = torch.zeros(8, device=dev()), torch.ones(8, device=dev())
    mean, invstd = ops.bn_stats(z.to(dev()), EPS, rm, rv, None, MOMENTUM)
    assert float(x.mean(0).min()) > 1000.0
    assert relerr(mean, x.mean(0)) < TOL and relerr(invstd, 1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS)) < TOL
    assert relerr(rv, 0.9 + 0.1 * x.var(0, unbiased=True)) < TOL


def test_batch_norm_refuses_one_row():
    ops = ops_mod()
    v = torch.ones(8, device=dev())
    with pytest.raises(RuntimeError, match="at least two rows"):
        ops.batch_norm(torch.zeros(1, 8, device=dev()), v, v, v.clone(), v.clone(), None)


# ---------------------------------------------------------------------------------------------------- PReLU
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (4, 16, 16, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [False, True], ids=["prelu", "relu"])
def test_prelu(shape, relu):
    ops = ops_mod()
    tag = "irse/prelu/%s" % "x".join(map(str, shape))
    C = shape[-1]
    x, dy = rnd(tag + "/x", shape), rnd(tag + "/dy", shape)
    x[0, 1] = 0.0       # a row of exact zeros: torch's rule there is the slope's branch
    slope = 0.25 * (1.0 + 0.5 * uni(tag + "/a", (C,)))
    slope[1::2] *= -1.0
    xr = x.double().requires_grad_()
    if relu:
        yr = F.relu(xr)
    else:
        ar = slope.double().requires_grad_()
        yr = F.prelu(xr.reshape(-1, C), ar).reshape(shape)
    (yr * dy.double()).sum().backward()
    ref = dict(y=yr.detach(), dx=xr.grad)
    if not relu:
        ref["da"] = ar.grad

    def run(bucket):
        xg = g(x)
        sl = None if relu else g(slope)
        if bucket and sl is not None:
            sl.grad = torch.full_like(sl.detach(), 0.25)
        y = ops.prelu(xg, sl)
        y.backward(dy.to(dev()))
        out = dict(y=y.detach(), dx=xg.grad)
        if sl is not None:
            out["da"] = sl.grad - 0.25 if bucket else sl.grad
        return out
    close(twice(lambda: run(False)), ref)
    close(twice(lambda: run(True)), ref)


# ---------------------------------------------------------------------------------------------------- SE tail, subsample
@pytest.mark.parametrize("N,Ho,Wo,C,ss", [(2, 1, 1, 8, 1), (3, 3, 5, 8, 1), (2, 3, 5, 64, 2), (2, 1, 1, 64, 2), (4, 4, 4, 64, 1)])
def test_se_tail_backward(N, Ho, Wo, C, ss):
    ops = ops_mod()
    tag = "irse/se/%d_%d_%d_%d_%d" % (N, Ho, Wo, C, ss)
    res, gate = rnd(tag + "/res", (N, Ho, Wo, C)), rnd(tag + "/gate", (N, C), 2.0)
    sc, dout = rnd(tag + "/sc", (N, Ho * ss, Wo * ss, C)), rnd(tag + "/dout", (N, Ho, Wo, C))
    r, gt, s = (t.double().requires_grad_() for t in (res, gate, sc))
    out = r * torch.sigmoid(gt)[:, None, None, :] + s[:, ::ss, ::ss]
    (out * dout.double()).sum().backward()
    ref = dict(out=out.detach(), dres=r.grad, dgate=gt.grad, dsc=s.grad)

    def run():
        rg, gg, sg = g(res), g(gate), g(sc)
        o = ops.se_tail_train(rg, gg, sg, ss)
        dres, dgate, dsc = torch.autograd.grad(o, (rg, gg, sg), dout.to(dev()))
        return dict(out=o.detach(), dres=dres, dgate=dgate, dsc=dsc)
    got = twice(run)
    close(got, ref)
    if ss == 2:     # the zeros of the scatter are written, not assumed
        assert float(got["dsc"][:, 1::2].abs().max()) == 0.0 and float(got["dsc"][:, :, 1::2].abs().max()) == 0.0


@pytest.mark.parametrize("N,H,W,C", [(2, 4, 6, 8), (3, 2, 2, 64)])
def test_subsample2(N, H, W, C):
    ops = ops_mod()
    from optimalstrategiesagainstgenerativeattacks_amd import _lib
    tag = "irse/sub/%d_%d_%d_%d" % (N, H, W, C)
    x, dy = rnd(tag + "/x", (N, H, W, C)), rnd(tag + "/dy", (N, H // 2, W // 2, C))

    def run():
        xg = g(x)
        y = ops.subsample2(xg)
        (dx,) = torch.autograd.grad(y, xg, dy.to(dev()))
        return dict(y=y.detach(), dx=dx)
    got = twice(run)
    want = torch.zeros(N, H, W, C)
    want[:, ::2, ::2] = dy
    assert torch.equal(got["y"].cpu(), x[:, ::2, ::2]) and torch.equal(got["dx"].cpu(), want)
    # the backward writes every element: into a buffer full of NaN
    dx = torch.full((N, H, W, C), float("nan"), device=dev())
    dyg = dy.to(dev())
    _lib.check(_lib.load().gim_subsample2_bwd(dyg.data_ptr(), dx.data_ptr(), N, H, W, C, ops._stream()), "subsample2_bwd")
    assert torch.equal(dx.cpu(), want)


# ---------------------------------------------------------------------------------------------------- dropout
def test_dropout():
    ops = ops_mod()
    n, p = 1 << 16, 0.4
    x = (rnd("irse/drop/x", (n,)).abs() + 0.5).to(dev())
    assert torch.equal(ops.dropout(x, 0.0, 5, 0), x)
    xg = x.clone().requires_grad_()
    y = ops.dropout(xg, p, 5, 1000)
    keep = y != 0
    share = float(keep.float().mean())
    sigma = math.sqrt(p * (1 - p) / n)
    print("    kept share %.5f (expected %.2f, sigma %.2e)" % (share, 1 - p, sigma))
    assert abs(share - (1 - p)) < 4 * sigma
    assert relerr(y[keep], x[keep] / (1 - p)) < 1e-6
    (dx,) = torch.autograd.grad(y, xg, torch.ones_like(x))
    assert torch.equal(dx != 0, keep) and relerr(dx[keep], torch.full_like(dx[keep], 1 / (1 - p))) < 1e-6
    assert torch.equal(ops.dropout(x, p, 5, 1000), y.detach())
    other = ops.dropout(x, p, 5, 1000 + n) != 0
    agree = float((other == keep).float().mean())       # independent masks agree on p^2 + (1 - p)^2 = 0.52 of the elements
    assert abs(agree - (p * p + (1 - p) ** 2)) < 0.02, agree
    assert not torch.equal(ops.dropout(x, p, 6, 1000) != 0, keep)
    # the mask of element i at offset o is the mask of element i - 4 at offset o + 4: the counter is offset + index
    assert torch.equal((ops.dropout(x, p, 5, 1004) != 0)[:-4], keep[4:])


# ---------------------------------------------------------------------------------------------------- embedding and head
def test_l2norm_rows_backward():
    ops = ops_mod()
    x, dy = rnd("irse/l2/x", (3, 512)), rnd("irse/l2/dy", (3, 512))
    xr = x.double().requires_grad_()
    yr = xr / xr.norm(dim=1, keepdim=True)
    (yr * dy.double()).sum().backward()

    def run():
        xg = g(x)
        y = ops.l2norm_rows_train(xg)
        return dict(y=y.detach(), dx=torch.autograd.grad(y, xg, dy.to(dev()))[0])
    close(twice(run), dict(y=yr.detach(), dx=xr.grad))


@pytest.mark.parametrize("E,N", [(512, 11), (16, 1000)])
def test_col_l2norm(E, N):
    ops = ops_mod()
    k, dn = uni("irse/col/%d/k" % N, (E, N)), rnd("irse/col/%d/dn" % N, (E, N))
    kr = k.double().requires_grad_()
    nr = kr / kr.norm(dim=0, keepdim=True)
    (nr * dn.double()).sum().backward()

    def run():
        kg = g(k)
        n = ops.col_l2norm(kg)
        return dict(n=n.detach(), dk=torch.autograd.grad(n, kg, dn.to(dev()))[0])
    close(twice(run), dict(n=nr.detach(), dk=kr.grad))


def margin_reference(cos, label, s=64.0, m=0.5):
    """arcface/models.py:190-207 restated on fp64 torch."""
    c = cos.clamp(-1, 1)
    ctm = c * math.cos(m) - torch.sqrt(1 - c * c) * math.sin(m)
    ctm = torch.where(c - math.cos(math.pi - m) <= 0, c - math.sin(m) * m, ctm)
    onehot = F.one_hot(label, cos.shape[1]).bool()
    return torch.where(onehot, ctm, c) * s


@pytest.mark.parametrize("N", [11, 1000])
def test_arc_margin(N):
    ops = ops_mod()
    B = 5
    tag = "irse/margin/%d" % N
    cos = 0.6 * uni(tag + "/cos", (B, N))
    label = torch.tensor([(3 * i) % N for i in range(B)])
    th = math.cos(math.pi - 0.5)      # -0.8776
    for b, v in enumerate([0.7, -0.95, 0.1, th - 0.06, th + 0.06]):      # label cosines on both sides of the threshold
        cos[b, label[b]] = v
    cos[0, 1], cos[1, 2] = 1.25, -1.5      # beyond the clamp: no gradient there
    # (exactly +-1 is left out: the kernel passes the gradient there as clamp does, while autograd of the reference's expression gives
    # NaN in every column - 0 * inf through the sqrt(1 - c^2) that only the label column uses)
    cr = cos.double().requires_grad_()
    lab = cr.detach()[torch.arange(B), label]
    assert float((lab.abs() - 1).abs().min()) >= 0.05 - 1e-6 and float((lab - th).abs().min()) >= 0.05 and (lab < th).any() and (lab > th).any()
    dout = rnd(tag + "/dout", (B, N))
    outr = margin_reference(cr, label)
    (outr * dout.double()).sum().backward()
    assert float(cr.grad[0, 1]) == 0.0 and float(cr.grad[1, 2]) == 0.0

    def run():
        cg = g(cos)
        out = ops.arc_margin(cg, label.to(dev()), 64.0, 0.5)
        return dict(out=out.detach(), dcos=torch.autograd.grad(out, cg, dout.to(dev()))[0])
    got = twice(run)
    close(got, dict(out=outr.detach(), dcos=cr.grad))
    assert float(got["dcos"][0, 1]) == 0.0 and float(got["dcos"][1, 2]) == 0.0


@pytest.mark.parametrize("N", [11, 1000])
def test_softmax_ce(N):
    ops = ops_mod()
    B = 6
    tag = "irse/ce/%d" % N
    logits = 64.0 * 0.6 * uni(tag + "/x", (B, N))
    label = torch.tensor([(3 * i) % N for i in range(B)])
    logits[1, label[1]] = 60.0                              # row 1: the label wins
    logits[2, 7], logits[2, 3] = 50.0, 50.0                 # row 2: a tie of the two largest, the first one (3) counts
    label[2] = 3
    logits[3, 7], logits[3, 3] = 50.0, 50.0                 # row 3: the same tie, the label is the second one
    label[3] = 7
    dl = rnd(tag + "/dl", (B,))
    xr = logits.double().requires_grad_()
    lr = F.cross_entropy(xr, label, reduction="none")
    (lr * dl.double()).sum().backward()
    am = xr.detach().argmax(1)
    want = torch.tensor([float(int(torch.nonzero(xr.detach()[b] == xr.detach()[b].max())[0]) == int(label[b])) for b in range(B)])
    assert want[1] == 1.0 and want[2] == 1.0 and want[3] == 0.0 and am.shape == (B,)

    def run():
        xg = g(logits)
        loss, correct = ops.softmax_ce(xg, label.to(dev()))
        assert not correct.requires_grad
        return dict(loss=loss.detach(), correct=correct, dx=torch.autograd.grad(loss, xg, dl.to(dev()))[0])
    got = twice(run)
    close(got, dict(loss=lr.detach(), dx=xr.grad))
    assert torch.equal(got["correct"].cpu(), want)


def test_margin_softmax_loss_and_accuracy():
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import margin_softmax_loss, top1_accuracy
    logits = 64.0 * 0.6 * uni("irse/loss/x", (8, 11))
    label = torch.tensor(af.proto_labels())
    xg = g(logits)
    loss = margin_softmax_loss(xg, label.to(dev()))
    assert tuple(loss.shape) == (1,)
    loss.backward(torch.ones(1, device=dev()))
    xr = logits.double().requires_grad_()
    lr = F.cross_entropy(xr, label)
    lr.backward()
    assert relerr(loss, lr.detach().view(1)) < TOL and relerr(xg.grad, xr.grad) < TOL
    acc = top1_accuracy(xg, label.to(dev()))
    assert acc.dim() == 0 and float(acc) == float((xr.detach().argmax(1) == label).double().mean())


# ---------------------------------------------------------------------------------------------------- the SE linears on the existing path
@pytest.mark.parametrize("cin,cout", [(64, 4), (4, 64), (512, 32), (32, 512)])
def test_se_linears_on_the_convolution_path(cin, cout):
    """No new kernel: the two 1x1 convolutions of the SE bottleneck on a [4, C] squeeze, as ops.linear on a 2-D weight and as
    ops.conv2d on the [N, 1, 1, C] map with the nn.Conv2d weight (the form irse_unit_train uses)."""
    ops = ops_mod()
    tag = "irse/selin/%d_%d" % (cin, cout)
    x, w, dy = rnd(tag + "/x", (4, cin)), rnd(tag + "/w", (cout, cin), cin ** -0.5), rnd(tag + "/dy", (4, cout))
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = xr @ wr.t()
    (yr * dy.double()).sum().backward()
    ref = dict(y=yr.detach(), dx=xr.grad, dw=wr.grad)

    def run_linear():
        xg, wg = g(x), g(w)
        y = ops.linear(xg, wg)
        dx, dw = torch.autograd.grad(y, (xg, wg), dy.to(dev()))
        return dict(y=y.detach(), dx=dx, dw=dw)

    def run_conv():
        xg, wg = g(x), g(w.view(cout, cin, 1, 1))
        y = ops.conv2d(xg.view(4, 1, 1, cin), wg)
        dx, dw = torch.autograd.grad(y, (xg, wg), dy.to(dev()).view(4, 1, 1, cout))
        return dict(y=y.detach().view(4, cout), dx=dx, dw=dw.reshape(cout, cin))
    prev = ops.set_deterministic(True)
    try:
        close(twice(run_linear), ref)
        close(twice(run_conv), ref)
    finally:
        ops.set_deterministic(prev)


# ---------------------------------------------------------------------------------------------------- units against the reference
def _unit(cin, depth, stride, body_idx):
    from optimalstrategiesagainstgenerativeattacks_amd import baselines as bl
    ent, pre = af.unit_entries(body_idx)
    unit = bl._Unit(cin, depth, stride)
    unit.load_state_dict(bf.filled_state(ent, af.UNIT_TAG, torch.float32, prefix=pre), strict=True)
    return unit.to(dev())


@pytest.mark.parametrize("cin,depth,stride,body_idx", af.UNITS, ids=[af.unit_name(*u[:3]) for u in af.UNITS])
def test_unit_vs_reference_golden(cin, depth, stride, body_idx):
    """bottleneck_IR_SE in training mode, N = 4 on 8 x 8: output, input gradient and every parameter gradient at 1e-4, the running
    statistics at max(3 x the reference's own fp32-vs-fp64 deviation, 3e-5)."""
    from optimalstrategiesagainstgenerativeattacks_amd.baseline_training import irse_unit_train
    ops = ops_mod()
    gold = load_npz("arcface_train.npz")
    name = af.unit_name(cin, depth, stride)
    x, dy = af.unit_input(cin, depth, stride)
    x, dy = torch.from_numpy(x).float().to(dev()), torch.from_numpy(dy).float().to(dev())

    def run():
        unit = _unit(cin, depth, stride, body_idx)
        xg = ops.to_nhwc(x).detach().requires_grad_()
        out = irse_unit_train(unit, xg)
        out.backward(ops.to_nhwc(dy))
        res = {"out": ops.to_nchw(out.detach()), "dx": ops.to_nchw(xg.grad)}
        for k, p in unit.named_parameters():
            res["grad/" + k] = p.grad
        for k, v in unit.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                res["run/" + k] = v
            elif k.endswith("num_batches_tracked"):
                assert int(v) == 8, k
        return res
    prev = ops.set_deterministic(True)      # the convolutions' weight gradients combine by atomics otherwise
    try:
        got = twice(run)
    finally:
        ops.set_deterministic(prev)
    largest = max(float(gold["%s/gradnorm/%s" % (name, k[5:])]) for k in got if k.startswith("grad/"))
    for k, v in got.items():
        ref = gold["%s/%s" % (name, k)]
        if k.startswith("grad/"):
            idx = torch.from_numpy(af.sample_index(v.numel())).to(dev())
            norm = float(gold["%s/gradnorm/%s" % (name, k[5:])])
            if norm < af.SMALL_REL * largest:      # mathematically zero (a constant in front of a BatchNorm): rounding noise only
                e, bound = float(v.double().norm()) / largest, 1e-5
            else:
                # the sampled elements against the reference's, relative to the rms of the whole tensor
                rms = norm / math.sqrt(v.numel())
                e = float((v.reshape(-1)[idx].double().cpu() - torch.from_numpy(ref).double()).norm()) / (rms * math.sqrt(len(ref)))
                bound = BLOCK
        else:
            e = relerr(v, ref)
            bound = max(3.0 * float(gold["floor/%s/%s" % (name, k)]), TOL) if k.startswith("run/") else BLOCK
        print("    %-40s %.3e (bound %.1e)" % (k, e, bound))
        assert e < bound, (k, e, bound)
