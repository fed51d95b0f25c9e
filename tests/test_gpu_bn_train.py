"""ops.bn_relu_maxpool2 (BatchNorm2d with batch statistics -> ReLU -> MaxPool2d(2), csrc/bn_train.hip), ops.bn_stats and
ops.absdiff_train against fp64 torch on the CPU: F.batch_norm(training=True) -> relu -> max_pool2d(2), autograd for the gradients.

Inputs lie on a grid: z = k / 8 with integer k in [-32, 32], distinct within every pooling window, gamma = +-(1 + 0.3 u) (negative on a
quarter of the channels), beta = 0.3 u.  That keeps the arg-max and ReLU decisions away from ties: ONE window routed differently moves
dz by ~5e-3 relative, which no fp32 bound would absorb.  Every case first asserts, on the fp64 reference, that the two largest
normalised values of every window are more than 1e-4 apart and that every window maximum is more than 1e-4 away from 0 (the tie case
states its ties instead).  Every test is a single shot."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import portable_fill as pf
from tests.helpers import T, relerr

TOL = 3e-5          # relative L2, fp32 kernels against fp64 (tests/test_gpu_baselines.py, tests/test_gpu_ops.py)
TOL_DZ = 2e-4       # a norm layer's dx (test_instance_norm)
TOL_MAX = 2e-4      # largest single-element error relative to the largest reference element
POINTWISE = 1e-6    # a few fp32 roundings
MARGIN = 1e-4
MOMENTUM, EPS = 0.1, 1e-5

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def grid_map(tag, N, H, W, C):
    """z [N, H, W, C] = k / 8, k integer in [-32, 32], the four values of every 2x2 window of a channel distinct."""
    order = np.argsort(pf.uniform(tag + "/k", (N, H // 2, W // 2, C, 65)), axis=-1)[..., :4] - 32      # [N, Ho, Wo, C, 4]
    k = order.reshape(N, H // 2, W // 2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)
    return T(k / 8.0)


def affine(tag, C):
    gamma = 1.0 + 0.3 * pf.uniform(tag + "/gamma", (C,))
    gamma[1::4] *= -1.0
    return T(gamma), T(0.3 * pf.uniform(tag + "/beta", (C,)))


_REF = {}


def reference(tag, z, gamma, beta, dp, ties=False):
    """fp64 torch on the CPU (NCHW inside); everything comes back NHWC.  Computed once per tag."""
    if tag in _REF:
        return _REF[tag]
    C = z.shape[3]
    x = z.permute(0, 3, 1, 2).contiguous().requires_grad_()
    g, b = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    rm, rv = T(0.2 * pf.uniform(tag + "/rm", (C,))), T(1.0 + 0.5 * np.abs(pf.uniform(tag + "/rv", (C,))))
    rm0, rv0 = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm, rv, g, b, training=True, momentum=MOMENTUM, eps=EPS)
    p = F.max_pool2d(F.relu(y), 2)
    (p * dp.permute(0, 3, 1, 2)).sum().backward()
    # the decisions the kernels take must not hang on a rounding
    win = F.unfold(y.detach().reshape(-1, 1, *y.shape[2:]), 2, stride=2).sort(dim=1, descending=True).values   # [N * C, 4, windows]
    gap, absmax = float((win[:, 0] - win[:, 1]).min()), float(win[:, 0].abs().min())
    print("%s: smallest top-two gap %.3e, smallest |window max| %.3e" % (tag, gap, absmax))
    assert absmax > MARGIN and (ties or gap > MARGIN), (tag, gap, absmax)
    mean = x.detach().mean((0, 2, 3))
    var = x.detach().var((0, 2, 3), unbiased=False)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    _REF[tag] = dict(p=nhwc(p), dz=nhwc(x.grad), dgamma=g.grad, dbeta=b.grad, mean=mean, invstd=1.0 / torch.sqrt(var + EPS),
                     rm0=rm0, rv0=rv0, rm=rm, rv=rv)
    return _REF[tag]


def run(ops, z, gamma, beta, dp, rm0, rv0):
    d = dev()
    zg = z.float().to(d).requires_grad_()
    gg, bg = gamma.float().to(d).requires_grad_(), beta.float().to(d).requires_grad_()
    rm, rv = rm0.float().to(d), rv0.float().to(d)
    nbt = torch.tensor(7, dtype=torch.int64, device=d)
    p = ops.bn_relu_maxpool2(zg, gg, bg, rm, rv, nbt, MOMENTUM, EPS)
    dz, dgamma, dbeta = torch.autograd.grad(p, (zg, gg, bg), dp.float().to(d))
    mean, invstd = ops.bn_stats(zg.detach(), EPS)
    return dict(p=p.detach(), dz=dz, dgamma=dgamma, dbeta=dbeta, mean=mean, invstd=invstd, rm=rm, rv=rv, nbt=nbt)


def check_case(tag, z, gamma, beta, ties=False):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, W, C = z.shape
    dp = T(pf.uniform(tag + "/dp", (N, H // 2, W // 2, C)))
    ref = reference(tag, z, gamma, beta, dp, ties)
    got = run(ops, z, gamma, beta, dp, ref["rm0"], ref["rv0"])
    again = run(ops, z, gamma, beta, dp, ref["rm0"], ref["rv0"])
    errs = {k: relerr(got[k], ref[k]) for k in ("p", "dz", "dgamma", "dbeta", "mean", "invstd", "rm", "rv")}
    emax = float((got["p"].double().cpu() - ref["p"]).abs().max() / ref["p"].abs().max())
    print("%s: %s, p max element %.2e" % (tag, " ".join("%s %.2e" % kv for kv in errs.items()), emax))
    for k, e in errs.items():
        assert e < (TOL_DZ if k == "dz" else TOL), (tag, k, e)
    assert emax < TOL_MAX, (tag, emax)
    assert int(got["nbt"]) == 8
    for k in got:     # no float atomics anywhere: two runs are bit-identical
        assert torch.equal(got[k], again[k]), (tag, k)
    return got, ref


SHAPES = {
    "one_window": (1, 2, 2, 4),       # one window, one quad; M = 4, the smallest map: the unbiased M / (M - 1) = 4 / 3
    "rect": (3, 4, 8, 64),            # H != W
    "c132": (2, 2, 2, 132),           # a channel count that is no multiple of the workgroup's 64-channel block
    "slabs": (5, 16, 16, 64),         # M = 1280 rows: several slabs, the last groups of the combine empty
    "slabs65": (65, 16, 16, 4),       # 4160 pooled rows: 65 slabs, lane 0 of the backward sums' stage 2 adds two; 260 for the statistics
}
FILL = {"slabs": "#1"}      # fill names whose fp64 reference has the margins above ("bnt/slabs" itself has a window maximum of 4.5e-5)


@pytest.mark.parametrize("name", list(SHAPES))
def test_bn_relu_maxpool2_vs_fp64(name):
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, W, C = SHAPES[name]
    if name == "slabs":
        assert ops.bn_slabs(N * H * W) >= 3 and ops.bn_slabs(N * (H // 2) * (W // 2)) >= 2
    if name == "slabs65":
        assert ops.bn_slabs(N * H * W) == 260 and ops.bn_slabs(N * (H // 2) * (W // 2)) == 65
    tag = "bnt/" + name + FILL.get(name, "")
    check_case(tag, grid_map(tag, N, H, W, C), *affine(tag, C))


def test_bn_relu_maxpool2_adds_into_existing_grad():
    """gamma.grad and beta.grad exist (FusedAdam's bucket): the sums are ADDED there by the kernel and autograd gets None."""
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    N, H, W, C = SHAPES["rect"]
    tag = "bnt/rect"
    z, (gamma, beta) = grid_map(tag, N, H, W, C), affine(tag, C)
    dp = T(pf.uniform(tag + "/dp", (N, H // 2, W // 2, C)))
    ref = reference(tag, z, gamma, beta, dp)
    d = dev()
    zg = z.float().to(d).requires_grad_()
    gg, bg = gamma.float().to(d).requires_grad_(), beta.float().to(d).requires_grad_()
    gg.grad, bg.grad = torch.full_like(gg.detach(), 0.25), torch.full_like(bg.detach(), 0.25)
    rm, rv = ref["rm0"].float().to(d), ref["rv0"].float().to(d)
    p = ops.bn_relu_maxpool2(zg, gg, bg, rm, rv, torch.tensor(7, dtype=torch.int64, device=d), MOMENTUM, EPS)
    dz, dgamma, dbeta = torch.autograd.grad(p, (zg, gg, bg), dp.float().to(d), allow_unused=True)
    assert dgamma is None and dbeta is None
    for k, got, tol in (("dgamma", gg.grad - 0.25, TOL), ("dbeta", bg.grad - 0.25, TOL), ("dz", dz, TOL_DZ)):
        e = relerr(got, ref[k])
        print("%s bucket %s: %.2e" % (tag, k, e))
        assert e < tol, (k, e)


def test_offset_map_keeps_its_variance():
    """z + 1024: the spread is 2.3 on a level of 1024.  E[x^2] - E[x]^2 in fp32 has an absolute error of ~1e6 * 6e-8 * sqrt(M) there,
    a multiple of a tenth of the variance; sums about a shift taken from the data do not see the offset."""
    tag = "bnt/offset"
    got, ref = check_case(tag, grid_map(tag, 2, 8, 8, 8) + 1024.0, *affine(tag, 8))
    assert float(ref["mean"].min()) > 1000.0


def test_dead_channel_has_exactly_zero_gradient():
    """A channel with negative gamma whose every window maximum is <= 0: no pooled element passes the ReLU, so dbeta = dgamma = 0 and
    dz = s * (0 - 0 - xhat * 0) is exactly zero, not rounding noise."""
    tag = "bnt/dead"
    gamma, beta = affine(tag, 8)
    assert float(gamma[1]) < 0
    beta[1] = -10.0
    got, ref = check_case(tag, grid_map(tag, 2, 4, 4, 8), gamma, beta)
    assert float(ref["p"][..., 1].abs().max()) == 0.0
    assert float(got["p"][..., 1].abs().max()) == 0.0
    assert float(got["dz"][..., 1].abs().max()) == 0.0 and float(got["dgamma"][1]) == 0.0 and float(got["dbeta"][1]) == 0.0
    assert float(got["dz"][..., 0].abs().max()) > 0.0


def test_tie_goes_to_first_maximum():
    """Two equal maxima in every window: the gradient goes to the first one in row-major window order (torch.nn.MaxPool2d's rule) -
    after the affine, so for a negative gamma to the first of the two equal MINIMA of z."""
    tag = "bnt/tie"
    N, H, W, C = 2, 4, 4, 4
    windows = np.array([[3, 3, 1, 0], [0, 2, 2, 1], [1, 0, 4, 4], [2, 1, 2, 0],       # ties of the maximum of z
                        [-3, -3, 1, 0], [0, -2, -2, 1], [1, 0, -4, -4], [-2, 1, -2, 0]])  # ties of its minimum
    k = np.empty((N, H // 2, W // 2, C, 4))
    for i in range(N * (H // 2) * (W // 2)):
        for c in range(C):
            k.reshape(-1, C, 4)[i, c] = windows[(i + 3 * c) % 8] + (i % 3)
    z = T(k.reshape(N, H // 2, W // 2, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(N, H, W, C) / 8.0)
    gamma, beta = T(np.array([1.3, -1.1, 0.9, -1.2])), T(np.array([0.4, 0.5, 0.45, 0.35]))
    check_case(tag, z, gamma, beta, ties=True)


def test_absdiff_train():
    from optimalstrategiesagainstgenerativeattacks_amd import ops
    a64, b64, d64 = (T(pf.uniform("bnt/abs/" + nm, (6, 256))) for nm in "abd")
    b64[::3, ::5] = a64[::3, ::5]        # equal elements: gradient 0 (torch's abs')
    ar, br = a64.clone().requires_grad_(), b64.clone().requires_grad_()
    yr = (ar - br).abs()
    yr.backward(d64)
    a, b = a64.float().to(dev()).requires_grad_(), b64.float().to(dev()).requires_grad_()
    y = ops.absdiff_train(a, b)
    da, db = torch.autograd.grad(y, (a, b), d64.float().to(dev()))
    eq = (a64.float() == b64.float())
    assert int(eq.sum()) > 0
    for nm, got, ref in (("y", y, yr), ("da", da, ar.grad), ("db", db, br.grad)):
        e = relerr(got, ref)
        print("absdiff_train %s: %.2e" % (nm, e))
        assert e < POINTWISE, (nm, e)
    assert float(da.cpu()[eq].abs().max()) == 0.0 and float(db.cpu()[eq].abs().max()) == 0.0
    # the two halves of one matrix (the pair batch encoded in one pass)
    e = torch.cat([a.detach(), b.detach()], 0).requires_grad_()
    yh = ops.absdiff_halves(e)
    (ge,) = torch.autograd.grad(yh, e, d64.float().to(dev()))
    assert torch.equal(yh, y) and torch.equal(ge[:6], da) and torch.equal(ge[6:], db)
